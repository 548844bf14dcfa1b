// Exact binomial variates from counter-based Philox noise (sample.hip: the nodes of the multinomial splitting tree).
//
// A variate is a pure function of (N, p, seed, draw, node): its uniforms come from Philox blocks with the counter
// {node, draw low word, draw high word, BINOMIAL_TAG + attempt} under the key `seed`, so neither the launch shape nor
// the order in which threads run can change it.  Two regimes, both exact (no normal or Poisson approximation):
//   N min(p, 1-p) <  10   sequential inversion from k = 0 in f64, starting at q^N = exp(N log1p(-p))
//   N min(p, 1-p) >= 10   Hoermann's transformed rejection with squeeze (BTRS; W. Hoermann, "The generation of binomial random
//                         variates", J. Statist. Comput. Simul. 46 (1993) 101-110), acceptance test with Stirling tails of lgamma
// The attempts of one variate are capped (BINOMIAL_MAX_ATTEMPTS): reaching the cap sets *err and returns the mode -- there is no
// unbounded loop.  (BTRS accepts with probability > 0.7 per attempt; the inversion restarts only when rounding left its
// accumulated mass below a uniform within 1e-15 of 1.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rng.hpp"

namespace polee {

constexpr uint32_t BINOMIAL_TAG = 0x62690000u;  // counter word 3 = tag + attempt (the N(0,1) noise of rng.hpp uses 0x706f6c65)
constexpr int BINOMIAL_MAX_ATTEMPTS = 64;
constexpr double BINOMIAL_INVERSION_BELOW = 10.0;  // N p below this: inversion
constexpr int BINOMIAL_INVERSION_MAX_K = 96;       // P(X > 96 | N p < 10) < 1e-55: past it the uniform is drawn again

// A double strictly inside (0, 1) from two Philox words: (k + 1/2) 2^-52 with k the 52 bits w0[31:6] w1[31:6] -- an odd 53-bit
// significand, exact (the 24 bits of philox_u01f would put a floor of 6e-8 under every tail).
__host__ __device__ inline double philox_u01_53(uint32_t w0, uint32_t w1)
{
    const uint64_t k = ((uint64_t)(w0 >> 6) << 26) | (uint64_t)(w1 >> 6);
    return ((double)k + 0.5) * (1.0 / 4503599627370496.0);
}

// the two uniforms of attempt `attempt`
__host__ __device__ inline void binomial_uniforms(uint64_t seed, uint64_t draw, uint32_t node, int attempt, double *u, double *v)
{
    uint32_t c[4] = {node, (uint32_t)draw, (uint32_t)(draw >> 32), BINOMIAL_TAG + (uint32_t)attempt};
    philox4x32_10(c, seed);
    *u = philox_u01_53(c[0], c[1]);
    *v = philox_u01_53(c[2], c[3]);
}

// log(k!) - [ (k + 1/2) log(k + 1) - (k + 1) + log(2 pi) / 2 ]: the tail of Stirling's series at k + 1
__host__ __device__ inline double stirling_tail(double k)
{
    if (k < 10.0) {
        const int i = (int)k;  // (a chain of selects: no constant table in memory for a device function inlined into several kernels)
        return i == 0 ? 0.0810614667953272 : i == 1 ? 0.0413406959554092 : i == 2 ? 0.0276779256849983 :
               i == 3 ? 0.02079067210376509 : i == 4 ? 0.0166446911898211 : i == 5 ? 0.0138761288230707 :
               i == 6 ? 0.0118967099458917 : i == 7 ? 0.0104112652619720 : i == 8 ? 0.00925546218271273 : 0.00833056343336287;
    }
    const double k1 = k + 1.0, k1sq = k1 * k1;
    return (1.0 / 12.0 - (1.0 / 360.0 - 1.0 / 1260.0 / k1sq) / k1sq) / k1;
}

// One Binomial(N, p) variate; 0 <= N < 2^31, 0 <= p <= 1 (callers check).  *err is set (never cleared) when the attempts ran out.
__host__ __device__ inline int64_t binomial_draw(int64_t N, double p, uint64_t seed, uint64_t draw, uint32_t node, int *err)
{
    if (N <= 0 || p <= 0.0) return 0;
    if (p >= 1.0) return N;
    const bool flip = p > 0.5;
    const double pp = flip ? 1.0 - p : p, qq = 1.0 - pp, n = (double)N;
    int64_t k = -1;
    if (n * pp < BINOMIAL_INVERSION_BELOW) {
        const double f0 = exp(n * log1p(-pp)), s = pp / qq;
        const int64_t kmax = N < BINOMIAL_INVERSION_MAX_K ? N : BINOMIAL_INVERSION_MAX_K;
        for (int attempt = 0; attempt < BINOMIAL_MAX_ATTEMPTS && k < 0; ++attempt) {
            double u, v;
            binomial_uniforms(seed, draw, node, attempt, &u, &v);
            double f = f0;
            for (int64_t x = 0; x <= kmax; ++x) {
                if (u < f) {
                    k = x;
                    break;
                }
                u -= f;
                f *= s * ((n - (double)x) / ((double)x + 1.0));
            }
        }
    } else {
        const double spread = sqrt(n * pp * qq);
        const double b = 1.15 + 2.53 * spread;
        const double a = -0.0873 + 0.0248 * b + 0.01 * pp;
        const double c = n * pp + 0.5;
        const double vr = 0.92 - 4.2 / b;
        const double r = pp / qq;
        const double alpha = (2.83 + 5.1 / b) * spread;
        const double mode = floor((n + 1.0) * pp);
        for (int attempt = 0; attempt < BINOMIAL_MAX_ATTEMPTS && k < 0; ++attempt) {
            double u, v;
            binomial_uniforms(seed, draw, node, attempt, &u, &v);
            u -= 0.5;
            const double us = 0.5 - fabs(u);
            const double x = floor((2.0 * a / us + b) * u + c);
            if (us >= 0.07 && v <= vr) {  // the squeeze: inside the box under the hat that lies under the density
                k = (int64_t)x;
                break;
            }
            if (x < 0.0 || x > n) continue;
            const double lv = log(v * alpha / (a / (us * us) + b));
            const double bound = (mode + 0.5) * log((mode + 1.0) / (r * (n - mode + 1.0))) +
                                 (n + 1.0) * log((n - mode + 1.0) / (n - x + 1.0)) +
                                 (x + 0.5) * log(r * (n - x + 1.0) / (x + 1.0)) + stirling_tail(mode) + stirling_tail(n - mode) -
                                 stirling_tail(x) - stirling_tail(n - x);
            if (lv <= bound) k = (int64_t)x;
        }
    }
    if (k < 0) {  // the attempts ran out
        if (err) *err = 1;
        k = (int64_t)floor((n + 1.0) * pp);
    }
    return flip ? N - k : k;
}

}  // namespace polee

// The exact definition of the forest of `polee model random-forest`, shared by the device builder
// (forest.hip) and the host builder (forest_host.cpp): the bootstrap, the keyed bijection behind a node's candidate features, the
// order of floats and the score of a boundary.  Integers, Philox counters and f64 additions in a fixed order only: whoever follows
// these definitions gets the same forest bit for bit.
#pragma once
#include "rng.hpp"

#include <cmath>
#include <cstdint>

#include "../../include/polee_hip.h"

namespace polee {
namespace forest {

constexpr int FO_MAX_K = 16;
constexpr int32_t FO_MAX_TREES = 1 << 16;
// word 1 of a Philox counter names its use (a Feistel round adds its number 0..3)
constexpr uint32_t FO_TAG_BOOT = 0x626f6f74u;
constexpr uint32_t FO_TAG_FEISTEL = 0x66656900u;

__host__ __device__ inline uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// entry i of tree t's bootstrap sample: a row in [0, N)
__host__ __device__ inline uint32_t boot_row(uint64_t seed, uint32_t tree, uint32_t i, uint32_t N)
{
    uint32_t c[4] = {i, FO_TAG_BOOT, 0u, tree};
    philox4x32_10(c, seed);
    return mulhi32(c[0], N);
}

// half the width of the Feistel domain: the bit length of n-1 rounded up to even (at least 2), halved
__host__ __device__ inline int feistel_half_bits(uint32_t n)
{
    int b = 0;
    for (uint32_t m = n - 1; m; m >>= 1) ++b;
    if (b < 2) b = 2;
    return (b + 1) >> 1;
}

// Position `pos` of the bijection of [0, n) keyed by (seed, tree, node): a balanced 4-round Feistel network over 2 h bits whose round
// function is word 0 of the Philox block (half, tag + round, node, tree), cycle-walked until the value is below n.
__host__ __device__ inline uint32_t candidate_feature(uint64_t seed, uint32_t tree, uint32_t node, uint32_t n, uint32_t pos)
{
    const int h = feistel_half_bits(n);
    const uint32_t mask = (1u << h) - 1u;
    uint32_t v = pos;
    do {
        uint32_t L = v >> h, R = v & mask;
        for (uint32_t r = 0; r < 4; ++r) {
            uint32_t c[4] = {R, FO_TAG_FEISTEL + r, node, tree};
            philox4x32_10(c, seed);
            const uint32_t nr = L ^ (c[0] & mask);
            L = R;
            R = nr;
        }
        v = (L << h) | R;
    } while (v >= n);
    return v;
}

// unsigned keys in the order of the floats (-0 just below +0: equal as floats, so never a boundary)
__host__ __device__ inline uint32_t sortable_bits(uint32_t u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__host__ __device__ inline uint32_t unsortable_bits(uint32_t s) { return s ^ ((s >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// -(n_l H_l + n_r H_r) in nats from T[c] = c ln c: f64 additions in exactly this order
__host__ __device__ inline double boundary_score(const double *T, const int32_t *cl, const int32_t *tot, int k, int32_t nl, int32_t nr)
{
    double s = 0.0;
    for (int c = 0; c < k; ++c) {
        s += T[cl[c]];
        s += T[tot[c] - cl[c]];
    }
    s -= T[nl];
    s -= T[nr];
    return s;
}

__host__ __device__ inline double threshold_of(float lo, float hi) { return ((double)lo + (double)hi) / 2; }

// the sizes the options fix
inline int32_t nsub_of(int32_t n, double nsubfeatures)
{
    const double r = std::nearbyint(nsubfeatures * std::sqrt((double)n));  // (round half to even: the default rounding mode)
    if (!(r >= 1.0)) return 1;
    return r >= (double)n ? n : (int32_t)r;
}
inline int64_t nboot_of(int32_t N, double partial_sampling)
{
    const double r = std::floor(partial_sampling * (double)N);
    return r >= 1.0 ? (int64_t)r : 1;
}
// the table T[c] = c ln c, c = 0 .. count (T[0] = 0), computed on the host only
inline void clogc_table(double *T, int64_t count)
{
    T[0] = 0.0;
    for (int64_t c = 1; c <= count; ++c) T[c] = (double)c * std::log((double)c);
}

// what both builders refuse, with one message
const char *check_opts(const polee_forest_opts &o, int32_t n, int32_t k);
// node arrays nobody can walk out of: offsets from 0 and rising, no empty tree, features in -1 .. n-1, labels in 0 .. k-1, a node
// with a feature has two children in its tree, both after it.  On failure *bad_tree / *bad_node name the first offender.
bool nodes_ok(int32_t n, int32_t k, int32_t ntrees, const int64_t *tree_off, const int32_t *feature, const int32_t *left,
              const int32_t *right, const int32_t *label, int32_t *bad_tree, int64_t *bad_node);

}  // namespace forest
}  // namespace polee

// Wave64 reductions with DPP (no LDS traffic, unlike __shfl): shared by loglik.hip, regression.hip and em.hip.
// DPP reads of inactive lanes return 0 / stale data: call these with all 64 lanes active.
#pragma once
#include <hip/hip_runtime.h>

namespace polee {

// ---- wave-level sum via DPP (gfx9 row_shr / row_bcast), result valid in lane 63 ------------
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ inline float dpp_add(float v)
{
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, BANK_MASK, true);
    return v + __int_as_float(moved);
}
__device__ inline float wave_sum_to_lane63(float v)
{
    v = dpp_add<0x111, 0xf, 0xf>(v);  // row_shr:1   (inclusive scan inside each row of 16 lanes)
    v = dpp_add<0x112, 0xf, 0xf>(v);  // row_shr:2
    v = dpp_add<0x114, 0xf, 0xf>(v);  // row_shr:4
    v = dpp_add<0x118, 0xf, 0xf>(v);  // row_shr:8   -> lane 15 of every row holds the row total
    v = dpp_add<0x142, 0xa, 0xf>(v);  // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xc, 0xf>(v);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    return v;
}
// the same in f64: the two halves of every value move by the same DPP controls (a lane the move leaves out adds 0.0)
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ inline double dpp_add(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, BANK_MASK, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, BANK_MASK, true);
    return v + __hiloint2double(hi, lo);
}
__device__ inline double wave_sum_to_lane63(double v)
{
    v = dpp_add<0x111, 0xf, 0xf>(v);
    v = dpp_add<0x112, 0xf, 0xf>(v);
    v = dpp_add<0x114, 0xf, 0xf>(v);
    v = dpp_add<0x118, 0xf, 0xf>(v);
    v = dpp_add<0x142, 0xa, 0xf>(v);
    v = dpp_add<0x143, 0xc, 0xf>(v);
    return v;
}
// the same for 64-bit integers (xbuild.hip's counts): exact, so the order of the additions does not show
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ inline uint64_t dpp_add(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, BANK_MASK, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, BANK_MASK, true);
    return v + (((uint64_t)hi << 32) | (uint64_t)lo);
}
__device__ inline uint64_t wave_sum_to_lane63(uint64_t v)
{
    v = dpp_add<0x111, 0xf, 0xf>(v);
    v = dpp_add<0x112, 0xf, 0xf>(v);
    v = dpp_add<0x114, 0xf, 0xf>(v);
    v = dpp_add<0x118, 0xf, 0xf>(v);
    v = dpp_add<0x142, 0xa, 0xf>(v);
    v = dpp_add<0x143, 0xc, 0xf>(v);
    return v;
}
// the same for N values at once, step-major so that the N dependency chains interleave
template <int N>
__device__ inline void wave_sum_to_lane63_n(float (&v)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = dpp_add<0x111, 0xf, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = dpp_add<0x112, 0xf, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = dpp_add<0x114, 0xf, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = dpp_add<0x118, 0xf, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = dpp_add<0x142, 0xa, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = dpp_add<0x143, 0xc, 0xf>(v[i]);
}

// ---- KP sums at once with shuffles (classify.hip, tsne.hip) --------------------------------------
// p[0..KP) per lane -> the wave's sums: afterwards p[0] of every lane holds the sum of class lane / (64 / KP).  Halving exchange: at
// every step a lane keeps half of its values and receives its partner's partial of those, so KP - 1 + log2(64 / KP) shuffles in all.
template <int KP>
__device__ inline void wave_split_reduce(float (&p)[KP], int lane)
{
#pragma unroll
    for (int h = KP / 2; h >= 1; h >>= 1) {
        const int off = 64 * h / KP;
        const bool up = (lane & off) != 0;
#pragma unroll
        for (int c = 0; c < h; ++c) {
            const float send = up ? p[c] : p[c + h];
            const float keep = up ? p[c + h] : p[c];
            p[c] = keep + __shfl_xor(send, off, 64);
        }
    }
#pragma unroll
    for (int off = 32 / KP; off >= 1; off >>= 1) p[0] += __shfl_xor(p[0], off, 64);
}

}  // namespace polee

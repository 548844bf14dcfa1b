// The sampler's draws (rand!, src/approx-sampler.jl:37-44) block by block, shared by polee_sampler_draw and its siblings (vi.hip) and the
// streaming handle (sample.hip).  Draw d of a seed lives in the block of SAMPLER_BLOCK draws that starts at b0 = d - d % 8: its N(0,1)
// noise is philox_randn(sampler_block_seed(seed, b0), step 1, d - b0, node) -- so a draw is a function of (seed, d) alone, whatever
// part of its block a call asks for.
#pragma once
#include "common.hpp"
#include "ptt_internal.hpp"

namespace polee {

constexpr int32_t SAMPLER_BLOCK = 8;

inline uint64_t sampler_block_seed(uint64_t seed, uint64_t b0) { return seed + b0 * 0x9E3779B97F4A7C15ull; }

// Rows [r0, r0 + B) of the block that starts at draw b0 (b0 % 8 == 0, r0 + B <= 8) -> d_xs, row stride xs_rs (device, f32 [B][n]).
// d_mu, d_sigma, d_alpha: device f32 [n-1].  d_z0: device f32 [B][n-1], the caller's noise of THESE B draws, or null = the device
// RNG.  y_eps > 0 clamps y (the initial-value draws).  Queued on the context's stream; uses the tree's scratch.
polee_status sampler_block_device(polee_ptt *t, const float *d_mu, const float *d_sigma, const float *d_alpha, const float *d_z0,
                                  uint64_t seed, uint64_t b0, int32_t r0, int32_t B, double y_eps, float *d_xs, int64_t xs_rs);

}  // namespace polee

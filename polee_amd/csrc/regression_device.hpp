// Device helpers of the regression step (regression.hip): the layout of a block's flat parameter / noise vector (RegView), the
// elementwise math, one column's draws, Adam.
#pragma once
#include "common.hpp"

#include <cmath>

namespace polee {

constexpr int REG_MAXF = 16;    // factors (design-matrix columns)
constexpr int REG_MAXDEG = 32;  // kernel-regression hinges
constexpr int REG_BLOCK = 128;
constexpr int REG_SLOTS = 32;  // copies of every grid-wide accumulator (block b adds into copy b % 32): same-address
                               // float atomics from ~1.5 k blocks serialise, 32-way spreading removes that
constexpr float HALF_LOG2PI = 0.91893853320467274178f;
// Philox keys: every draw of regression.hip is keyed seed ^ REG_SEED_SALT; the noise of a rank's own samples also carries
// rank_salt (the latents every rank shares do not, so that replicas stay identical), the second block's REG_ISO_SALT on top
constexpr uint64_t REG_SEED_SALT = 0x7265677265737369ull;
constexpr uint64_t REG_RANK_SALT = 0xD1B54A32D192ED03ull;
constexpr uint64_t REG_ISO_SALT = 0x69736f666f726d73ull;

// Layout of the flat parameter / gradient vector and of the noise vector (include/polee_hip.h documents the order).
struct RegView {
    int32_t S, F, n, deg;
    int32_t use_distortion, point;
    float bias_loc0, bias_scale0, penalty;
    // > 0: x_scale ~ InverseGamma(fixed_ab, fixed_ab) instead of the kernel-regressed concentration / scale, and the
    // observation model stands alone (no sample scales, no scale-drift penalty, no likelihood term of its own): the
    // isoform block of the gene-isoform model (models/polee_regression.py:727-733), run with deg = 0
    float fixed_ab = 0.0f;
    // --- the joint model's variants (RNASeqJointLinearRegression, models/polee_regression.py:879-1283) ---
    int32_t levels = 2;       // 1: a horseshoe prior (one local scale level, :1009-1024) instead of horseshoe+; the local2 arrays stay in
                              //    the vector, unused (gradient 0)
    int32_t no_xs = 0;        // 1: no x_scale in this block (the splice-feature block: its observation lives on the transcripts)
    int32_t w_from_bias = 0;  // 1: the kernel-regression weights are functions of the SAMPLED bias (:1034-1035), not of x_bias_init
    float hc_scale = 1.0f;    // scale of the HalfCauchy prior on the mean-variance coefficients (10 in the joint model, :1037-1041)
    float bandwidth = 1.0f;
    const float *hinges = nullptr;  // (w_from_bias) device pointer, deg values
    __host__ __device__ int64_t Fn() const { return (int64_t)F * n; }
    __host__ __device__ int64_t o_dist() const { return 4; }
    __host__ __device__ int64_t o_conc() const { return 4 + (int64_t)F * deg; }
    __host__ __device__ int64_t o_scc() const { return o_conc() + deg; }
    __host__ __device__ int64_t o_cols() const { return o_scc() + deg; }  // 10 arrays [F][n]
    __host__ __device__ int64_t o_bias_loc() const { return o_cols() + 10 * Fn(); }
    __host__ __device__ int64_t o_bias_s() const { return o_bias_loc() + n; }
    __host__ __device__ int64_t o_xs_loc() const { return o_bias_loc() + 2 * (int64_t)n; }
    __host__ __device__ int64_t o_xs_s() const { return o_bias_loc() + 3 * (int64_t)n; }
    __host__ __device__ int64_t o_qx_loc() const { return o_bias_loc() + 4 * (int64_t)n; }
    __host__ __device__ int64_t o_qx_s() const { return o_qx_loc() + (int64_t)S * n; }
    __host__ __device__ int64_t num_params() const { return o_qx_s() + (int64_t)S * n; }
    // noise: 2 global, 5 arrays [F][n], x_bias [n], x_scale [n], x [S][n]
    __host__ __device__ int64_t e_cols() const { return 2; }
    __host__ __device__ int64_t e_bias() const { return 2 + 5 * Fn(); }
    __host__ __device__ int64_t e_xs() const { return e_bias() + n; }
    __host__ __device__ int64_t e_x() const { return e_bias() + 2 * (int64_t)n; }
    __host__ __device__ int64_t num_noise() const { return e_x() + (int64_t)S * n; }
    __host__ __device__ int num_red() const { return 1 + F * deg + 2 * deg; }
};

// The column kernels are VALU-bound (rocprofv3: ~7.4 k VALU instructions per thread with libm's exp / log / log1p and
// IEEE division), so the elementwise math uses the hardware transcendentals (v_exp_f32, v_log_f32, v_rcp_f32,
// v_sqrt_f32: 1 ulp each) -- errors of ~1e-6 relative, far inside the 1e-4 parity tolerance.
__device__ inline float fexp(float x) { return __expf(x); }
__device__ inline float flog(float x) { return __logf(x); }
__device__ inline float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ inline float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
// log1p(t), 0 <= t <= 1, with full relative accuracy for small t (log(1 + t) would round 1 + t)
__device__ inline float flog1p01(float t) { return t < 1e-3f ? t * (1.0f - t * (0.5f - t * (1.0f / 3.0f))) : flog(1.0f + t); }
__device__ inline float softplusf(float x) { return fmaxf(x, 0.0f) + flog1p01(fexp(-fabsf(x))); }
__device__ inline float sigmoidf(float x) { return frcp(1.0f + fexp(-x)); }
// lgamma(x) and psi(x), x > 0, together: the recurrences lgamma(x) = lgamma(x+1) - log x, psi(x) = psi(x+1) - 1/x up to
// x >= 8 (one log of the running product), then the Stirling / asymptotic series (truncation < 1e-8 at x = 8)
__device__ inline void lgamma_digamma(float x, float &lg, float &psi)
{
    float prod = 1.0f, r = 0.0f;
    while (x < 8.0f) {
        prod *= x;
        r -= frcp(x);
        x += 1.0f;
    }
    const float i = frcp(x), i2 = i * i, lx = flog(x);
    psi = r + lx - 0.5f * i - i2 * (1.0f / 12.0f - i2 * (1.0f / 120.0f - i2 * (1.0f / 252.0f)));
    lg = (x - 0.5f) * lx - x + HALF_LOG2PI + i * (1.0f / 12.0f - i2 * (1.0f / 360.0f - i2 * (1.0f / 1260.0f))) - flog(prod);
}

// one draw of SoftplusNormal(loc, softplus(sraw)) (src/polee.py:24-33) and its share of log q
struct SpDraw {
    float z, sg, eps, s, sgs, logq;
};
__device__ inline SpDraw sp_draw(float loc, float sraw, float eps)
{
    SpDraw d;
    d.eps = eps;
    d.s = softplusf(sraw);
    d.sgs = sigmoidf(sraw);
    const float u = loc + d.s * eps;
    d.z = softplusf(u);
    d.sg = sigmoidf(u);
    d.logq = -0.5f * eps * eps - flog(d.s) - HALF_LOG2PI + softplusf(-u);  // - log sigmoid(u)
    return d;
}
// G = d(-log p)/dz  ->  d loss / d loc, d loss / d sraw
__device__ inline void sp_grad(const SpDraw &d, float G, float &gloc, float &gs)
{
    const float a = G * d.sg - (1.0f - d.sg);
    gloc = a;
    gs = (a * d.eps - frcp(d.s)) * d.sgs;
}
// -log InverseGamma(0.5, 0.5)(z), -log HalfNormal(1)(z)
__device__ inline float nlp_ig_half(float z)
{
    return -(0.5f * -0.69314718055994530942f - 0.57236494292470008707f - 1.5f * flog(z) - 0.5f * frcp(z));
}
__device__ inline float nlp_halfnormal(float z) { return 0.22579135264472743236f + 0.5f * z * z; }  // -0.5 log(2/pi)

// One column's draws of the observation model for the noise eps (v: the block's layout): the coefficient of factor f,
// w = loc + softplus(s) eps; the same plus its distortion term sum_d c[f][d] W[d][j] (DT hinges at compile time, 0 = v.deg);
// the bias; x_scale.
__device__ inline float draw_w(const RegView &v, const float *__restrict__ p, const float *__restrict__ eps, int f, int64_t j)
{
    const int64_t Fn = v.Fn(), idx = (int64_t)f * v.n + j;
    return p[v.o_cols() + 8 * Fn + idx] + softplusf(p[v.o_cols() + 9 * Fn + idx]) * eps[v.e_cols() + 4 * Fn + idx];
}
template <int DT>
__device__ inline float draw_weff(const RegView &v, const float *__restrict__ p, const float *__restrict__ eps,
                                  const float *__restrict__ W, int f, int64_t j)
{
    constexpr int UD = DT ? DT : 1;
    const int deg = DT ? DT : v.deg, n = v.n;
    const float w = draw_w(v, p, eps, f, j);
    float wd = 0.0f;
    if (v.use_distortion) {
#pragma unroll UD
        for (int d = 0; d < deg; ++d) wd += p[v.o_dist() + f * deg + d] * W[(int64_t)d * n + j];
    }
    return w + wd;
}
__device__ inline float draw_bias(const RegView &v, const float *__restrict__ p, const float *__restrict__ eps, int64_t j)
{
    return p[v.o_bias_loc() + j] + softplusf(p[v.o_bias_s() + j]) * eps[v.e_bias() + j];
}
__device__ inline float draw_xscale(const RegView &v, const float *__restrict__ p, const float *__restrict__ eps, int64_t j)
{
    return softplusf(p[v.o_xs_loc() + j] + softplusf(p[v.o_xs_s() + j]) * eps[v.e_xs() + j]);
}

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// (advances the clock: Adam's bias-corrected rate at the new step)
__device__ inline float adam_tick(uint32_t *tick, float lr)
{
    const double t = (double)(++tick[0]);
    return (float)((double)lr * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
}
// tf.optimizers.Adam: theta -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps); returns the step, lr_t the bias-corrected rate
// (0.1f and 0.001f are the literals, not 1 - b: those round differently)
__device__ inline float adam_step(float &m, float &vv, float gi, float lr_t)
{
    const float mi = 0.9f * m + 0.1f * gi;
    const float vi = 0.999f * vv + 0.001f * gi * gi;
    m = mi;
    vv = vi;
    return lr_t * mi / (sqrtf(vi) + 1e-7f);
}

}  // namespace polee

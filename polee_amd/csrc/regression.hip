// The regression model's variational step, device resident.
// Replaces RNASeqLinearRegression.model_fn / variational_model_fn / fit (models/polee_regression.py:18-340):
// TensorFlow-Probability's JointDistributionCoroutine pair + tfp.vi.fit_surrogate_posterior(sample_size = 1,
// Adam(2e-3)) become hand-derived gradients of
//     loss = log q(z) - log p(z),   z one reparameterised draw of the surrogate posterior,
// with the approximate likelihood term supplied by polee_approx_logprob_device (approx.hip).
//
// One step:
//   noise    : Philox normals for every latent (or host-provided noise)           -> eps   [num_noise]
//   lse      : t_s = logsumexp_j qx_loc[s][j] (the scale-drift penalty's value)   -> lse   [S]
//   sample x : x = qx_loc + softplus(qx_softplus_scale) eps                       -> x     [S][n]
//   lik      : approximate likelihood of x with d/dx                              -> lp [S], glik [S][n]
//   data     : one thread per feature j over this rank's samples: observation-model sums (F+2 per column),
//              gradients of qx_loc / qx_softplus_scale, the samples' loss terms           -> stats [(F+2) n + 32]
//   (samples sharded over ranks: ONE all-reduce of stats, polee_regression_set_comm)
//   columns  : one thread per feature j: draws the horseshoe+ scales, w, x_bias, x_scale of its column,
//              evaluates its share of log q - log p and all per-column gradients from stats; block-reduces
//              the pieces shared by columns (global scale, distortion, mean-variance coefficients)
//   finish   : the few global parameters
//   adam     : Keras Adam over the flat parameter vector
// Everything is O((F + S) n) bytes per step (cache / latency bound): no roofline claim.
//
// Blocks: a handle holds two RegBlocks -- a RegView (the layout of a flat parameter / noise vector over n columns) with the
// buffers that go with it: parameters, gradient, Adam moments, noise, the data pass's stats and the prior pass's accumulators.
// `main` is the model polee_regression_create describes.  `iso` is what a polee_regression_set_*_likelihood call adds, and
// IsoKind says which: gene (no view: a tail of isoform means and values, reg_iso_grad_kernel), gene-isoform (a view over the
// transcripts, run through the same data / column / finish kernels) or joint (a view over the splice features followed by a
// transcript tail, reg_joint_*_kernel).  A set-up call builds its block locally and moves it into the handle as its last act.
#include "common.hpp"
#include "comm_internal.hpp"
#include "regression_device.hpp"
#include "rng.hpp"
#include "wave.hpp"

#include <cmath>
#include <memory>
#include <type_traits>

namespace polee {

// Device-side clock of the fit, so that a whole step is one replayable hipGraph: tick[0] = Adam step t, tick[1] =
// slot of the loss trace; seed_dev[0] = seed of the fit, lr_t[0] = Adam's step size at t.
__global__ void reg_tick_kernel(uint32_t *tick, float *lr_t, float lr) { lr_t[0] = adam_tick(tick, lr); }

// seed / step: immediates, or (tick != nullptr) read from the device clock
__global__ void reg_noise_kernel(int64_t count, uint64_t seed, uint32_t step, const uint64_t *seed_dev,
                                 const uint32_t *tick, uint64_t salt, float *eps, uint32_t tick_ahead = 0u)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q * 4 >= count) return;
    if (tick) {
        seed = seed_dev[0];
        step = tick[0] + tick_ahead;  // (tick_ahead = 1: the clock is advanced later in the step, reg_finish_kernel)
    }
    seed ^= salt;
    float z[4];
    philox_randn4(seed ^ REG_SEED_SALT, step, (uint32_t)(q >> 32), (uint32_t)q, z);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (q * 4 + i < count) eps[q * 4 + i] = z[i];
}

// One launch per step for both noise segments and the draw of x (round 6: the tick, two noise launches and reg_sample_x_kernel
// were four ~5 us launches of a ~290 us step).  The step number is the device clock's NEXT value, tick[0] + 1: the clock
// itself is advanced by reg_finish_kernel, the step's last single-workgroup launch in front of Adam.  Segment 0 = the latents
// every rank shares (salt 0), segment 1 = the x noise of this rank's samples (salted): the same Philox blocks, in the same
// places, as two reg_noise_kernel launches.  A thread of segment 1 also writes x = qx_loc + softplus(qx_scale) eps for its
// four entries (x == nullptr: point estimates, no draw).
__global__ void reg_draw_kernel(RegView v, int64_t shared, int64_t own, const uint64_t *seed_dev, const uint32_t *tick, uint64_t salt,
                                const float *__restrict__ p, float *__restrict__ eps, float *__restrict__ x)
{
    const int64_t nq0 = (shared + 3) / 4;
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool seg1 = q >= nq0;
    if (seg1) q -= nq0;
    const int64_t count = seg1 ? own : shared;
    if (q * 4 >= count) return;
    const uint64_t seed = seed_dev[0] ^ (seg1 ? salt : (uint64_t)0);
    const uint32_t step = tick[0] + 1u;
    float z[4];
    philox_randn4(seed ^ REG_SEED_SALT, step, (uint32_t)(q >> 32), (uint32_t)q, z);
    float *e = eps + (seg1 ? shared : 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (q * 4 + i < count) {
            e[q * 4 + i] = z[i];
            if (seg1 && x) x[q * 4 + i] = p[v.o_qx_loc() + q * 4 + i] + softplusf(p[v.o_qx_s() + q * 4 + i]) * z[i];
        }
}

// t_s = logsumexp_j qx_loc[s][j]   (qx_sample_scale, models/polee_regression.py:300-301)
__global__ __launch_bounds__(1024) void reg_lse_kernel(RegView v, const float *p, float *lse)
{
    __shared__ float red[16];
    const float *row = p + v.o_qx_loc() + (int64_t)blockIdx.x * v.n;
    float m = -INFINITY;
    for (int j = threadIdx.x; j < v.n; j += 1024) m = fmaxf(m, row[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
    __syncthreads();
    float s = 0.0f;
    for (int j = threadIdx.x; j < v.n; j += 1024) s += expf(row[j] - m);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int i = 0; i < 16; ++i) t += red[i];
        lse[blockIdx.x] = m + logf(t);
    }
}

// The same once a nearby shift is known (the previous step's value: Adam moves qx_loc by ~lr per step), so that the
// row can be spread over many blocks: acc[s] += sum exp(qx_loc - lse_prev[s]); then lse = lse_prev + log acc.
__global__ __launch_bounds__(256) void reg_lse_accum_kernel(RegView v, const float *p, const float *lse, float *acc)
{
    __shared__ float red[4];
    const int s = blockIdx.y;
    const float *row = p + v.o_qx_loc() + (int64_t)s * v.n;
    const float c = lse[s];
    float t = 0.0f;
    const int64_t j0 = (int64_t)blockIdx.x * 4096, j1 = j0 + 4096 < v.n ? j0 + 4096 : v.n;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) t += expf(row[j] - c);
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&acc[s], red[0] + red[1] + red[2] + red[3]);
}
__global__ void reg_lse_finish_kernel(int S, float *lse, float *acc)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    lse[s] += logf(acc[s]);
    acc[s] = 0.0f;
}

__global__ void reg_sample_x_kernel(RegView v, const float *p, const float *eps, float *x)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)v.S * v.n) return;
    x[i] = p[v.o_qx_loc() + i] + softplusf(p[v.o_qx_s() + i]) * eps[v.e_x() + i];
}

// Likelihood of RNASeqNormalTranscriptLinearRegression (models/polee_regression.py:490-531): the point estimates
// v [S][n] ~ Normal(log softmax(x), sigma).  One block per sample: lp[s] and glik = d lp / d x.
__global__ __launch_bounds__(1024) void reg_normal_lik_kernel(int n, const float *__restrict__ x,
                                                               const float *__restrict__ v,
                                                               const float *__restrict__ sigma, float *lp, float *glik)
{
    __shared__ float red[16];
    const int s = blockIdx.x, tid = threadIdx.x;
    const float *xr = x + (int64_t)s * n, *vr = v + (int64_t)s * n, *sr = sigma + (int64_t)s * n;
    float *gr = glik + (int64_t)s * n;
    auto block_sum = [&](float val) {
        val = wave_sum(val);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = val;
        __syncthreads();
        float t = 0.0f;
        for (int i = 0; i < 16; ++i) t += red[i];
        return t;
    };
    float m = -INFINITY;
    for (int j = tid; j < n; j += 1024) m = fmaxf(m, xr[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
    float se = 0.0f;
    for (int j = tid; j < n; j += 1024) se += expf(xr[j] - m);
    const float lse = m + logf(block_sum(se));
    float sr_sum = 0.0f, l = 0.0f;
    for (int j = tid; j < n; j += 1024) {
        const float is = 1.0f / sr[j], d = (vr[j] - (xr[j] - lse)) * is;
        sr_sum += d * is;
        l += -0.5f * d * d - logf(sr[j]) - HALF_LOG2PI;
    }
    const float R = block_sum(sr_sum);
    const float L = block_sum(l);
    if (tid == 0) lp[s] = L;
    for (int j = tid; j < n; j += 1024) {
        const float is = 1.0f / sr[j];
        gr[j] = (vr[j] - (xr[j] - lse)) * is * is - expf(xr[j] - lse) * R;
    }
}

// ---- gene-level model (RNASeqGeneLinearRegression, models/polee_regression.py:533-600): the features are genes and
// the likelihood is reached through within-gene isoform log-expression x_isoform [S][nt] with
//   x_isoform_mean ~ Normal(0, 2) [nt],  x_isoform ~ Normal(x_isoform_mean, 1),  both with Normal surrogates.
// Isoform block of parameters: mean_loc [nt], mean_softplus_scale [nt], iso_loc [S][nt], iso_softplus_scale [S][nt];
// noise: mean [nt], iso [S][nt].
// (also the joint model's transcript tail, which has the same layout: scale loc / s [nt], x_iso loc / s [S][nt])
__global__ void reg_iso_sample_kernel(int S, int nt, const float *ip, const float *ieps, float *xi)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, snt = (int64_t)S * nt;
    if (i >= snt) return;
    xi[i] = ip[2 * (int64_t)nt + i] + softplusf(ip[2 * (int64_t)nt + snt + i]) * ieps[nt + i];
}
// gi = d lp / d x_isoform (from the gene-level likelihood); thread per transcript
__global__ __launch_bounds__(256) void reg_iso_grad_kernel(int S, int nt, const float *__restrict__ ip,
                                                           const float *__restrict__ ieps,
                                                           const float *__restrict__ gi, float *__restrict__ ig,
                                                           float *loss_slots)
{
    const int64_t ii = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, snt = (int64_t)S * nt;
    const bool live = ii < nt;
    const int64_t i = live ? ii : nt - 1;
    const float *loc = ip + 2 * (int64_t)nt, *sr = loc + snt;
    const float ms_raw = ip[nt + i], ms = softplusf(ms_raw), me = ieps[i];
    const float m = ip[i] + ms * me;
    float loss = -0.5f * me * me - flog(ms) - HALF_LOG2PI;               // log q(mean)
    loss += 0.125f * m * m + 0.69314718055994530942f + HALF_LOG2PI;      // -log Normal(0, 2)(mean)
    float Gm = 0.25f * m;
    for (int s = 0; s < S; ++s) {
        const int64_t o = (int64_t)s * nt + i;
        const float sraw = sr[o], sx = softplusf(sraw), e = ieps[nt + o];
        const float d = loc[o] + sx * e - m;
        loss += 0.5f * d * d + HALF_LOG2PI;                              // -log Normal(mean, 1)(x_isoform)
        loss += -0.5f * e * e - flog(sx) - HALF_LOG2PI;                  // log q(x_isoform)
        Gm -= d;
        const float Gx = d - gi[o];
        if (live) {
            ig[2 * (int64_t)nt + o] = Gx;
            ig[2 * (int64_t)nt + snt + o] = (Gx * e - frcp(sx)) * sigmoidf(sraw);
        }
    }
    if (live) {
        ig[i] = Gm;
        ig[nt + i] = (Gm * me - frcp(ms)) * sigmoidf(ms_raw);
    }
    loss = wave_sum_to_lane63(live ? loss : 0.0f);
    if ((threadIdx.x & 63) == 63) atomicAdd(&loss_slots[blockIdx.x % REG_SLOTS], loss);
}

// ---- joint model (RNASeqJointLinearRegression, models/polee_regression.py:879-1283): beside the gene block a SPLICE block --
// horseshoe coefficients w_splice [F][P] and a bias ~ Normal(0, 10) over P splice features (:1062-1087), whose linear
// predictor reaches the transcripts through the 0/1 feature matrix (:1089-1108): x_iso_loc[s][t] = sum of (F w + b)[s][p] over
// the features p of transcript t; x_iso_scale ~ HalfCauchy(0, 1) [nt] (:1110-1112), x_iso ~ Normal(x_iso_loc, x_iso_scale)
// (:1114-1116), and the gene-level likelihood of (x_gene, x_iso) (:1118-1121).  The splice features' coefficients are a
// RegView over P "columns" (levels = 1, no_xs) run through the column / finish kernels; the transcripts' part -- x_iso_scale
// (SoftplusNormal surrogate) and x_iso (Normal surrogate) -- is the kernel below.  Transcript part of the parameter block:
// x_iso_scale_loc [nt], x_iso_scale_softplus_scale [nt], x_iso_loc [S][nt], x_iso_softplus_scale [S][nt]; noise: scale [nt],
// x_iso [S][nt] (x_iso is drawn by reg_iso_sample_kernel).
// mu[s][p] = x_splice_bias[p] + sum_f F[s][f] w_splice[f][p] at the block's draw (thread per feature)
__global__ void reg_joint_mean_kernel(RegView vs, int S, const float *__restrict__ sp, const float *__restrict__ seps,
                                      const float *__restrict__ design, float *__restrict__ mu)
{
    const int64_t pidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pidx >= vs.n) return;
    const float b = draw_bias(vs, sp, seps, pidx);
    float w[REG_MAXF];
    for (int f = 0; f < vs.F; ++f) w[f] = draw_w(vs, sp, seps, f, pidx);
    for (int s = 0; s < S; ++s) {
        float m = b;
        for (int f = 0; f < vs.F; ++f) m += design[s * vs.F + f] * w[f];
        mu[(int64_t)s * vs.n + pidx] = m;
    }
}
// thread per transcript: x_iso_scale's draw, the observation term of its S values, log q of both, their gradients (gi = d lp /
// d x_iso from the gene-level likelihood); resid[s][t] = (x_iso - x_iso_loc) / x_iso_scale^2 goes on to the features
__global__ __launch_bounds__(256) void reg_joint_iso_kernel(int S, int nt, int P, const float *__restrict__ jp,
                                                            const float *__restrict__ jeps, const float *__restrict__ gi,
                                                            const float *__restrict__ mu, const int32_t *__restrict__ t_ptr,
                                                            const int32_t *__restrict__ t_feat, float *__restrict__ jg,
                                                            float *__restrict__ resid, float *loss_slots)
{
    const int64_t ii = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, snt = (int64_t)S * nt;
    const bool live = ii < nt;
    const int64_t i = live ? ii : nt - 1;
    const float *loc = jp + 2 * (int64_t)nt, *sr = loc + snt;
    const SpDraw xs = sp_draw(jp[i], jp[nt + i], jeps[i]);
    const float z = xs.z, iz = frcp(z), iz2 = iz * iz, lz = flog(z);
    float loss = xs.logq + 0.45158270528945486473f + log1pf(z * z);  // log q - log HalfCauchy(0, 1)
    float Gz = 2.0f * z / (1.0f + z * z);
    const int32_t f0 = t_ptr[i], f1 = t_ptr[i + 1];
    for (int s = 0; s < S; ++s) {
        const int64_t o = (int64_t)s * nt + i;
        float m = 0.0f;
        for (int32_t q = f0; q < f1; ++q) m += mu[(int64_t)s * P + t_feat[q]];
        const float sraw = sr[o], sx = softplusf(sraw), e = jeps[nt + o];
        const float d = loc[o] + sx * e - m;
        const float a = d * iz2;
        loss += 0.5f * d * a + lz + HALF_LOG2PI;              // -log Normal(x_iso_loc, x_iso_scale)(x_iso)
        loss += -0.5f * e * e - flog(sx) - HALF_LOG2PI;       // log q(x_iso)
        Gz += iz - d * a * iz;
        const float Gx = a - gi[o];
        if (live) {
            jg[2 * (int64_t)nt + o] = Gx;
            jg[2 * (int64_t)nt + snt + o] = (Gx * e - frcp(sx)) * sigmoidf(sraw);
            resid[o] = a;
        }
    }
    if (live) {
        float a, c;
        sp_grad(xs, Gz, a, c);
        jg[i] = a;
        jg[nt + i] = c;
    }
    loss = wave_sum_to_lane63(live ? loss : 0.0f);
    if ((threadIdx.x & 63) == 63) atomicAdd(&loss_slots[blockIdx.x % REG_SLOTS], loss);
}
// thread per splice feature: what the transcripts say about its column (the `stats` rows the column kernel reads)
__global__ void reg_joint_agg_kernel(int S, int nt, int P, int F, const float *__restrict__ resid,
                                     const float *__restrict__ design, const int32_t *__restrict__ p_ptr,
                                     const int32_t *__restrict__ p_trans, float *__restrict__ stats)
{
    const int64_t pidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pidx >= P) return;
    float gacc[REG_MAXF], sum_a = 0.0f;
    for (int f = 0; f < F; ++f) gacc[f] = 0.0f;
    const int32_t q0 = p_ptr[pidx], q1 = p_ptr[pidx + 1];
    for (int s = 0; s < S; ++s) {
        float a = 0.0f;
        for (int32_t q = q0; q < q1; ++q) a += resid[(int64_t)s * nt + p_trans[q]];
        sum_a += a;
        for (int f = 0; f < F; ++f) gacc[f] -= design[s * F + f] * a;
    }
    for (int f = 0; f < F; ++f) stats[(int64_t)f * P + pidx] = gacc[f];
    stats[(int64_t)F * P + pidx] = sum_a;
    stats[(int64_t)(F + 1) * P + pidx] = 0.0f;
}

// ---- data pass: what the S (local) samples say about each column ------------------------------------------
// stats [F+2][n] + REG_SLOTS:  rows 0..F-1  sum_s design[s][f] d(-log p_x)/d x_loc[s][j];  row F  sum_s (x - mu)/x_scale^2;
// row F+1  sum_s d(-log p_x)/d x_scale;  last REG_SLOTS values (summed by the reader)  loss terms of the samples (observation model, log q of x,
// scale-drift penalty, -likelihood).  These are sums over samples: with the samples sharded over ranks ONE all-reduce
// of this buffer is the only exchange of a step.  Also writes d loss / d qx_loc, qx_softplus_scale.
// (FT, DT: compile-time F and degree, 0 = run-time; fixed trip counts let the compiler issue a column's loads together)
template <int FT, int DT>
__global__ __launch_bounds__(REG_BLOCK) void reg_data_kernel(RegView v, const float *__restrict__ p,
                                                             const float *__restrict__ eps,
                                                             const float *__restrict__ design,
                                                             const float *__restrict__ W, const float *__restrict__ ss,
                                                             const float *__restrict__ x, const float *__restrict__ glik,
                                                             const float *__restrict__ lse, const float *__restrict__ lp,
                                                             float *__restrict__ g, float *__restrict__ stats)
{
    __shared__ float s_weff[FT ? FT : REG_MAXF][REG_BLOCK], s_gacc[FT ? FT : REG_MAXF][REG_BLOCK];
    const int tid = threadIdx.x;
    const int64_t jj = (int64_t)blockIdx.x * REG_BLOCK + tid;
    const bool live = jj < v.n;
    const int64_t j = live ? jj : v.n - 1;  // dead lanes recompute the last column and contribute nothing
    constexpr int UF = FT ? FT : 1;  // unroll count
    const int F = FT ? FT : v.F, n = v.n;
#pragma unroll UF
    for (int f = 0; f < F; ++f) {
        s_weff[f][tid] = draw_weff<DT>(v, p, eps, W, f, j);
        s_gacc[f][tid] = 0.0f;
    }
    const float b = draw_bias(v, p, eps, j);
    const float xsz = draw_xscale(v, p, eps, j);
    const float inv = frcp(xsz), inv2 = inv * inv, lxs = flog(xsz);
    const float ipen2 = 1.0f / (v.penalty * v.penalty);
    const bool sub = v.fixed_ab > 0.0f;  // (then ss, x, lse are null: x is recomputed from its surrogate)
    float loss = 0.0f, sum_a = 0.0f, sum_xs = 0.0f;
#pragma unroll 2  // (the samples' loads are independent: two in flight per lane)
    for (int s = 0; s < v.S; ++s) {
        float xl = b;
#pragma unroll UF
        for (int f = 0; f < F; ++f) xl += design[s * F + f] * s_weff[f][tid];
        const int64_t sj = (int64_t)s * n + j;
        const float xv = v.point ? p[v.o_qx_loc() + sj]
                                 : (sub ? p[v.o_qx_loc() + sj] + softplusf(p[v.o_qx_s() + sj]) * eps[v.e_x() + sj] : x[sj]);
        const float d = xv - (xl - (sub ? 0.0f : ss[s]));
        const float a = d * inv2;
        loss += 0.5f * d * a + lxs + HALF_LOG2PI;
        sum_xs += inv - d * a * inv;
        sum_a += a;
#pragma unroll UF
        for (int f = 0; f < F; ++f) s_gacc[f][tid] -= design[s * F + f] * a;
        float gl = 0.0f, gs = 0.0f;
        if (!v.point) {
            const float sraw = p[v.o_qx_s() + sj], sx = softplusf(sraw), e = eps[v.e_x() + sj];
            const float Gx = a - glik[sj];
            gl = sub ? Gx : Gx + lse[s] * ipen2 * fexp(p[v.o_qx_loc() + sj] - lse[s]);
            gs = (Gx * e - frcp(sx)) * sigmoidf(sraw);
            loss += -0.5f * e * e - flog(sx) - HALF_LOG2PI;
        }
        if (live) g[v.o_qx_loc() + sj] = gl, g[v.o_qx_s() + sj] = gs;
    }
    if (live) {
#pragma unroll UF
        for (int f = 0; f < F; ++f) stats[(int64_t)f * n + j] = s_gacc[f][tid];
        stats[(int64_t)F * n + j] = sum_a;
        stats[(int64_t)(F + 1) * n + j] = sum_xs;
    }
    loss = wave_sum(live ? loss : 0.0f);
    if (blockIdx.x == 0 && tid == 0 && !v.point && !sub)
        for (int s = 0; s < v.S; ++s) {  // per-sample terms: scale-drift penalty, approximate likelihood
            const float t = lse[s] / v.penalty;
            loss += 0.5f * t * t + logf(v.penalty) + HALF_LOG2PI - (lp ? lp[s] : 0.0f);
        }
    if ((tid & 63) == 0) atomicAdd(&stats[(int64_t)(F + 2) * n + (blockIdx.x % REG_SLOTS)], loss);
}

// ---- prior pass: everything that does not depend on which samples a rank holds, combined with the (summed) stats
// acc: loss (double [REG_SLOTS]); small [REG_SLOTS][num_red]: [0] sum (1 - r^2), then d/d(distortion_c) [F][deg], then the sums feeding
// d/d(concentration_c) [deg] and d/d(scale_c) [deg]
template <int FT, int DT>
__global__ __launch_bounds__(REG_BLOCK) void reg_cols_kernel(RegView v, const float *__restrict__ p,
                                                             const float *__restrict__ eps,
                                                             const float *__restrict__ W,
                                                             const float *__restrict__ stats, float *__restrict__ g,
                                                             double *loss_acc, float *small)
{
    __shared__ float s_red[1 + REG_MAXF * REG_MAXDEG + 2 * REG_MAXDEG];
    __shared__ float s_cc[REG_MAXDEG], s_sc[REG_MAXDEG];
    const int tid = threadIdx.x;
    const int64_t jj = (int64_t)blockIdx.x * REG_BLOCK + tid;
    const bool live = jj < v.n;
    const int64_t j = live ? jj : v.n - 1;
    constexpr int UF = FT ? FT : 1, UD = DT ? DT : 1;  // unroll counts
    const int F = FT ? FT : v.F, deg = DT ? DT : v.deg, n = v.n;
    const int64_t Fn = v.Fn();
    const int nred = v.num_red();
    const float lv = live ? 1.0f : 0.0f;
    const int lane = tid & 63;
    for (int i = tid; i < nred; i += REG_BLOCK) s_red[i] = 0.0f;
    if (tid < deg) {
        s_cc[tid] = softplusf(p[v.o_conc() + tid]);
        s_sc[tid] = softplusf(p[v.o_scc() + tid]);
    }
    __syncthreads();

    float loss = 0.0f, S1 = 0.0f;
    // global horseshoe scale (every thread recomputes the two scalars)
    const SpDraw gv = sp_draw(p[0], p[1], eps[0]), gn = sp_draw(p[2], p[3], eps[1]);
    const float gscale = gn.z * fsqrt(gv.z);

    // ---- horseshoe+ scales and w of every factor
#pragma unroll UF
    for (int f = 0; f < F; ++f) {
        const int64_t idx = (int64_t)f * n + j;
        const float *pc = p + v.o_cols() + idx;
        const float *ec = eps + v.e_cols() + idx;
        float *gc = g + v.o_cols() + idx;
        const SpDraw l1v = sp_draw(pc[0 * Fn], pc[1 * Fn], ec[0 * Fn]);
        const SpDraw l1n = sp_draw(pc[2 * Fn], pc[3 * Fn], ec[1 * Fn]);
        SpDraw l2v = sp_draw(pc[4 * Fn], pc[5 * Fn], ec[2 * Fn]);
        SpDraw l2n = sp_draw(pc[6 * Fn], pc[7 * Fn], ec[3 * Fn]);
        const bool two = v.levels > 1;
        if (!two) {  // horseshoe: no second local scale
            l2v.z = l2n.z = 1.0f;
            l2v.logq = l2n.logq = 0.0f;
        }
        const float sraw_w = pc[9 * Fn], s_w = softplusf(sraw_w), e_w = ec[4 * Fn];
        const float w = pc[8 * Fn] + s_w * e_w;
        const float sw = (l1n.z * fsqrt(l1v.z)) * (l2n.z * fsqrt(l2v.z)) * gscale;
        const float isw = frcp(sw), r = w * isw, q = 1.0f - r * r;
        S1 += q;
        loss += l1v.logq + l1n.logq + l2v.logq + l2n.logq + (-0.5f * e_w * e_w - flog(s_w) - HALF_LOG2PI);
        loss += nlp_ig_half(l1v.z) + nlp_halfnormal(l1n.z) + (two ? nlp_ig_half(l2v.z) + nlp_halfnormal(l2n.z) : 0.0f);
        loss += 0.5f * r * r + flog(sw) + HALF_LOG2PI;
        float a, b;
        float iz = frcp(l1v.z);
        sp_grad(l1v, iz * (1.5f + 0.5f * q - 0.5f * iz), a, b);  // 1.5/z - 0.5/z^2 + 0.5 q/z
        if (live) gc[0 * Fn] = a, gc[1 * Fn] = b;
        sp_grad(l1n, l1n.z + q * frcp(l1n.z), a, b);
        if (live) gc[2 * Fn] = a, gc[3 * Fn] = b;
        iz = frcp(l2v.z);
        sp_grad(l2v, iz * (1.5f + 0.5f * q - 0.5f * iz), a, b);
        if (live) gc[4 * Fn] = two ? a : 0.0f, gc[5 * Fn] = two ? b : 0.0f;
        sp_grad(l2n, l2n.z + q * frcp(l2n.z), a, b);
        if (live) gc[6 * Fn] = two ? a : 0.0f, gc[7 * Fn] = two ? b : 0.0f;
        const float gacc = stats[idx];
        const float Gw = r * isw + gacc;
        if (live) {
            gc[8 * Fn] = Gw;
            gc[9 * Fn] = (Gw * e_w - frcp(s_w)) * sigmoidf(sraw_w);
        }
        if (v.use_distortion) {
#pragma unroll UD
            for (int d = 0; d < deg; ++d) {
                const float t = wave_sum_to_lane63(lv * W[(int64_t)d * n + j] * gacc);
                if (lane == 63) atomicAdd(&s_red[1 + f * deg + d], t);
            }
        }
    }

    // ---- x_bias, x_scale
    const float s_b = softplusf(p[v.o_bias_s() + j]), e_b = eps[v.e_bias() + j];
    const float b = p[v.o_bias_loc() + j] + s_b * e_b;
    loss += -0.5f * e_b * e_b - flog(s_b) - HALF_LOG2PI;
    const float db = (b - v.bias_loc0) / v.bias_scale0;
    float Gb = db / v.bias_scale0 - stats[(int64_t)F * n + j];
    loss += 0.5f * db * db + logf(v.bias_scale0) + HALF_LOG2PI;
    float g_alpha = 0.0f, g_beta = 0.0f;
    // the kernel-regression weights of this column: precomputed from x_bias_init (W), or -- the joint model -- functions of
    // the sampled bias b (src/polee.py:36-47): k_d = clip(exp(-((b - h_d) / bw)^2), 1e-10, 1), w_d = k_d / sum k
    // (only the run-time-shape instance <0, 0> carries this variant: the fixed-shape instances of the transcript model keep
    // their register budget; the host launches <0, 0> for a view with w_from_bias)
    constexpr bool WB = FT == 0 && DT == 0;
    float wcol[WB ? REG_MAXDEG : 1], dl[WB ? REG_MAXDEG : 1];
    const bool wfb = WB && v.w_from_bias;
    if (wfb) {
        float tot = 0.0f;
        for (int d = 0; d < deg; ++d) {
            const float u = (b - v.hinges[d]) / v.bandwidth;
            const float k0 = fexp(-u * u);
            const bool clipped = k0 < 1e-10f;  // (the upper clip at 1 is never active: exp(-u^2) <= 1)
            wcol[d] = clipped ? 1e-10f : k0;
            dl[d] = clipped ? 0.0f : -2.0f * u / v.bandwidth;  // d log k_d / d b
            tot += wcol[d];
        }
        const float it = frcp(tot);
        for (int d = 0; d < deg; ++d) wcol[d] *= it;
    }
    if (!v.no_xs) {
        const SpDraw xs = sp_draw(p[v.o_xs_loc() + j], p[v.o_xs_s() + j], eps[v.e_xs() + j]);
        loss += xs.logq;
        float alpha = 0.0f, beta = 0.0f;
        if (wfb) {
            for (int d = 0; d < deg; ++d) {
                alpha += s_cc[d] * wcol[d];
                beta += s_sc[d] * wcol[d];
            }
        } else {
#pragma unroll UD
            for (int d = 0; d < deg; ++d) {
                const float wdj = W[(int64_t)d * n + j];
                alpha += s_cc[d] * wdj;
                beta += s_sc[d] * wdj;
            }
        }
        if (v.fixed_ab > 0.0f) alpha = beta = v.fixed_ab;
        const float inv = frcp(xs.z), inv2 = inv * inv, lxs = flog(xs.z);
        const float Gxs = (alpha + 1.0f) * inv - beta * inv2 + stats[(int64_t)(F + 1) * n + j];
        const float lbeta = flog(beta);
        float lg_alpha, psi_alpha;
        lgamma_digamma(alpha, lg_alpha, psi_alpha);
        loss += -(alpha * lbeta - lg_alpha - (alpha + 1.0f) * lxs - beta * inv);
        g_alpha = -lbeta + psi_alpha + lxs;
        g_beta = -alpha * frcp(beta) + inv;
        if (wfb) {  // d alpha / d b = sum_d cc_d w_d (l_d - lbar), lbar = sum_e w_e l_e; the same for beta
            float lbar = 0.0f, da = 0.0f, dbt = 0.0f;
            for (int d = 0; d < deg; ++d) lbar += wcol[d] * dl[d];
            for (int d = 0; d < deg; ++d) {
                da += s_cc[d] * wcol[d] * (dl[d] - lbar);
                dbt += s_sc[d] * wcol[d] * (dl[d] - lbar);
            }
            Gb += g_alpha * da + g_beta * dbt;
        }
        if (live) {
            float a, c;
            sp_grad(xs, Gxs, a, c);
            g[v.o_xs_loc() + j] = a;
            g[v.o_xs_s() + j] = c;
        }
    } else if (live) {
        g[v.o_xs_loc() + j] = 0.0f;
        g[v.o_xs_s() + j] = 0.0f;
    }
    if (live) {
        g[v.o_bias_loc() + j] = Gb;
        g[v.o_bias_s() + j] = (Gb * e_b - frcp(s_b)) * sigmoidf(p[v.o_bias_s() + j]);
    }

    // ---- block sums of what the columns share
#pragma unroll UD
    for (int d = 0; d < deg; ++d) {
        const float wdj = lv * (wfb ? wcol[WB ? d : 0] : W[(int64_t)d * n + j]);
        const float ta = wave_sum_to_lane63(wdj * g_alpha), tb = wave_sum_to_lane63(wdj * g_beta);
        if (lane == 63) {
            atomicAdd(&s_red[1 + F * deg + d], ta);
            atomicAdd(&s_red[1 + F * deg + deg + d], tb);
        }
    }
    S1 = wave_sum_to_lane63(lv * S1);
    loss = wave_sum_to_lane63(lv * loss);
    const int slot = blockIdx.x % REG_SLOTS;
    if (lane == 63) {
        atomicAdd(&s_red[0], S1);
        atomicAdd(&loss_acc[slot], (double)loss);
    }
    __syncthreads();
    for (int i = tid; i < nred; i += REG_BLOCK) atomicAdd(&small[(int64_t)slot * nred + i], s_red[i]);
}

// the global horseshoe scale and the distortion / mean-variance coefficients (one wave; lane i takes coefficient i)
// (it leaves every accumulator it has read at zero for the next step: no memsets between steps)
__global__ __launch_bounds__(64) void reg_finish_kernel(RegView v, const float *p, const float *eps, float *small,
                                                        float *stats, double *loss_acc, float *g, float *loss_out,
                                                        const float *extra_loss, uint32_t *tick, float *lr_t, float lr)
{
    const int lane = threadIdx.x, nred = v.num_red();
    if (tick && lane == 0) lr_t[0] = adam_tick(tick, lr);  // the device clock of fit(): this step's number and Adam's rate
    auto slots = [&](int i) {  // sum of accumulator i over its copies
        float t = 0.0f;
        for (int k = 0; k < REG_SLOTS; ++k) {
            t += small[(int64_t)k * nred + i];
            small[(int64_t)k * nred + i] = 0.0f;
        }
        return t;
    };
    double loss = 0.0;
    if (lane < REG_SLOTS) {  // the columns' terms + the samples' terms (summed over ranks)
        loss = loss_acc[lane] + (double)stats[(int64_t)(v.F + 2) * v.n + lane];
        loss_acc[lane] = 0.0;
        stats[(int64_t)(v.F + 2) * v.n + lane] = 0.0f;
    }
    if (lane == 0) {
        const float S1 = slots(0);
        const SpDraw gv = sp_draw(p[0], p[1], eps[0]), gn = sp_draw(p[2], p[3], eps[1]);
        loss += gv.logq + gn.logq + nlp_ig_half(gv.z) + nlp_halfnormal(gn.z);
        sp_grad(gv, 1.5f / gv.z - 0.5f / (gv.z * gv.z) + 0.5f * S1 / gv.z, g[0], g[1]);
        sp_grad(gn, gn.z + S1 / gn.z, g[2], g[3]);
    }
    for (int i = lane; i < v.F * v.deg; i += 64) {
        const float c = p[v.o_dist() + i];
        if (v.use_distortion) {
            g[v.o_dist() + i] = 2.0f * c / (0.01f + c * c) + slots(1 + i);
            loss += logf(3.14159265358979323846f * 0.1f) + log1pf(100.0f * c * c);
        } else
            g[v.o_dist() + i] = 0.0f;
    }
    for (int i = lane; i < 2 * v.deg; i += 64) {  // concentration_c then scale_c (adjacent in the vector)
        const int64_t o = v.o_conc() + i;
        const float c = softplusf(p[o]), hs = v.hc_scale;  // HalfCauchy(0, hs): -log p = -log(2 / (pi hs)) + log1p((c / hs)^2)
        g[o] = (2.0f * c / (hs * hs + c * c) + slots(1 + v.F * v.deg + i)) * sigmoidf(p[o]);
        loss += 0.45158270528945486473f + logf(hs) + log1pf((c / hs) * (c / hs));  // (0.4515... = -log(2/pi))
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o, 64);
    if (lane == 0) loss_out[0] = (float)(loss + (extra_loss ? (double)extra_loss[0] : 0.0));
}

__global__ void reg_adam_kernel(int64_t count, float *p, const float *g, float *m, float *vv, const float *lr_dev,
                                const float *loss, float *trace, uint32_t *tick)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && trace) trace[tick[1]++] = loss[0];  // (also when nothing is trainable: count may be 0)
    if (i >= count) return;
    p[i] -= adam_step(m[i], vv[i], g[i], lr_dev[0]);
}

// ---- classify (models/polee_regression.py:342-413): the design matrix of the testing samples is a latent variable, so the loss needs
// its gradient with respect to F[s][f].  F enters through the observation model only, x[s][j] ~ Normal(sum_f F[s][f] w_eff[f][j] + bias[j]
// - scale[s], x_scale[j]):  d(-log p)/dF[s][f] = -sum_j a[s][j] w_eff[f][j]  with a = (x - mu) / x_scale^2 -- the quantities of
// reg_data_kernel, recomputed here for the same draw (a kernel of its own: the hot data kernel stays as it is).  dF: [REG_SLOTS][S][F],
// block b adds into copy b % REG_SLOTS; the reader sums the copies.
__global__ __launch_bounds__(REG_BLOCK) void reg_design_grad_kernel(RegView v, const float *__restrict__ p, const float *__restrict__ eps,
                                                                   const float *__restrict__ design, const float *__restrict__ W,
                                                                   const float *__restrict__ ss, const float *__restrict__ x,
                                                                   float *__restrict__ dF)
{
    __shared__ float s_weff[REG_MAXF][REG_BLOCK];
    const int tid = threadIdx.x;
    const int64_t jj = (int64_t)blockIdx.x * REG_BLOCK + tid;
    const bool live = jj < v.n;
    const int64_t j = live ? jj : v.n - 1;
    const int F = v.F, n = v.n;
    for (int f = 0; f < F; ++f) s_weff[f][tid] = draw_weff<0>(v, p, eps, W, f, j);
    const float b = draw_bias(v, p, eps, j);
    const float xsz = draw_xscale(v, p, eps, j);
    const float inv = frcp(xsz), inv2 = inv * inv;
    float *out = dF + (int64_t)(blockIdx.x % REG_SLOTS) * v.S * F;
    for (int s = 0; s < v.S; ++s) {
        float xl = b;
        for (int f = 0; f < F; ++f) xl += design[s * F + f] * s_weff[f][tid];
        const int64_t sj = (int64_t)s * n + j;
        const float xv = v.point ? p[v.o_qx_loc() + sj] : x[sj];
        const float a = live ? (xv - (xl - ss[s])) * inv2 : 0.0f;
        for (int f = 0; f < F; ++f) {
            const float t = wave_sum(-a * s_weff[f][tid]);
            if ((tid & 63) == 0) atomicAdd(out + s * F + f, t);
        }
    }
}

// ---- latent design (RNASeqPCA, models/polee_pca.py:14-92): the design matrix is a parameter z [S][F] with a Normal(0, sigma) prior
// (latent_space_model_fn, :52-56) and a Deterministic surrogate (:58-59, log q = 0).  One workgroup, behind everything that reads the
// design in the step and behind reg_finish_kernel (which writes loss[0] and Adam's rate), in front of reg_adam_kernel (which copies
// loss[0] to the trace):  gz = sum of the slot copies of d(-log p)/dz + z / sigma^2 (the copies are left at zero for the next step: no
// memset between steps), loss += sum z^2 / (2 sigma^2) + log sigma + log(2 pi) / 2, and (update) Adam with reg_adam_kernel's constants
// and the step's bias-corrected rate lr_dev[0], z in place.
__global__ __launch_bounds__(256) void reg_latent_kernel(int SF, float *__restrict__ dz, float *__restrict__ z, float *__restrict__ m,
                                                         float *__restrict__ vv, float *__restrict__ gz, float inv_var, float nlp0,
                                                         const float *lr_dev, float *loss, int update)
{
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double l = 0.0;
    for (int i = tid; i < SF; i += 256) {
        float gi = 0.0f;
        for (int k = 0; k < REG_SLOTS; ++k) {
            gi += dz[(int64_t)k * SF + i];
            dz[(int64_t)k * SF + i] = 0.0f;
        }
        const float zi = z[i];
        gi += zi * inv_var;
        gz[i] = gi;
        l += (double)(0.5f * zi * zi * inv_var + nlp0);
        if (update) z[i] = zi - adam_step(m[i], vv[i], gi, lr_dev[0]);
    }
    l = wave_sum_to_lane63(l);
    if ((tid & 63) == 63) red[tid >> 6] = l;
    __syncthreads();
    if (tid == 0) loss[0] = (float)((double)loss[0] + red[0] + red[1] + red[2] + red[3]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// The reference's default degree (15) with up to four factors runs the data and column kernels with fixed trip counts, everything
// else at run-time shape <0, 0>: launch(FT, DT) is called with the pair as std::integral_constants.  fixed_ok = false forces <0, 0>.
template <class L>
void reg_dispatch(const RegView &v, bool fixed_ok, L &&launch)
{
    using std::integral_constant;
    const int ft = fixed_ok && v.deg == 15 && v.F <= 4 ? v.F : 0;
    if (ft == 1) launch(integral_constant<int, 1>{}, integral_constant<int, 15>{});
    else if (ft == 2) launch(integral_constant<int, 2>{}, integral_constant<int, 15>{});
    else if (ft == 3) launch(integral_constant<int, 3>{}, integral_constant<int, 15>{});
    else if (ft == 4) launch(integral_constant<int, 4>{}, integral_constant<int, 15>{});
    else launch(integral_constant<int, 0>{}, integral_constant<int, 0>{});
}

template <class T>
polee_status reg_zero(polee_ctx *ctx, DevBuf<T> &b)
{
    if (b.p) POLEE_HIP_TRY(ctx, hipMemsetAsync(b.p, 0, sizeof(T) * b.n, ctx->stream));
    return POLEE_OK;
}

// A block of variational parameters with everything a step keeps per block.  The view v lays out the front of p / g / m / vv
// (and of eps) over v.n columns; tail_params / tail_noise values that the view does not describe follow it in the same buffers.
// v.n == 0: no view, the block is its tail (and has no stats / small / acc / loss).
struct RegBlock {
    RegView v{};
    int64_t tail_params = 0, tail_noise = 0;
    DevBuf<float> p, g, m, vv, eps, stats, small, loss;
    DevBuf<double> acc;
    bool has_cols() const { return v.n > 0; }
    int64_t view_params() const { return has_cols() ? v.num_params() : 0; }
    int64_t view_noise() const { return has_cols() ? v.num_noise() : 0; }
    int64_t num_params() const { return view_params() + tail_params; }
    int64_t num_noise() const { return view_noise() + tail_noise; }
    int64_t num_stats() const { return (int64_t)(v.F + 2) * v.n + REG_SLOTS; }
    float *loss_slots() const { return stats.p + num_stats() - REG_SLOTS; }  // the samples' loss terms (see reg_data_kernel)

    // p0: the initial values of the view's parameters and of the tail; everything else is allocated and zeroed
    polee_status init(polee_ctx *ctx, const RegView &view, int64_t tail_p, int64_t tail_e, const std::vector<float> &p0)
    {
        v = view, tail_params = tail_p, tail_noise = tail_e;
        const size_t np = p0.size();  // == num_params()
        POLEE_TRY(p.upload(ctx, p0));
        for (DevBuf<float> *b : {&g, &m, &vv}) POLEE_TRY(b->alloc(ctx, np));
        POLEE_TRY(eps.alloc(ctx, (size_t)num_noise()));
        if (has_cols()) {
            POLEE_TRY(stats.alloc(ctx, (size_t)num_stats()));
            POLEE_TRY(small.alloc(ctx, (size_t)REG_SLOTS * v.num_red()));
            POLEE_TRY(acc.alloc(ctx, REG_SLOTS));
            POLEE_TRY(loss.alloc(ctx, 1));
        }
        for (DevBuf<float> *b : {&g, &m, &vv, &stats, &small}) POLEE_TRY(reg_zero(ctx, *b));
        POLEE_TRY(reg_zero(ctx, acc));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    }
    void take(RegBlock &o)  // (ownership moves here)
    {
        v = o.v, tail_params = o.tail_params, tail_noise = o.tail_noise;
        p.take(o.p), g.take(o.g), m.take(o.m), vv.take(o.vv), eps.take(o.eps);
        stats.take(o.stats), small.take(o.small), loss.take(o.loss), acc.take(o.acc);
    }
    // prior pass of the view: stats (summed over ranks) -> the gradients of everything its columns share and loss[0]
    // (+ extra_loss[0]); tick != nullptr: the finish kernel also advances the device clock.  A view with w_from_bias runs <0, 0>.
    void launch_prior(hipStream_t st, const float *W, const float *extra_loss, uint32_t *tick, float *lr_t, float lr) const
    {
        const dim3 grid((unsigned)ceil_div(v.n, REG_BLOCK));
        reg_dispatch(v, !v.w_from_bias, [&](auto ft, auto dt) {
            hipLaunchKernelGGL((reg_cols_kernel<decltype(ft)::value, decltype(dt)::value>), grid, dim3(REG_BLOCK), 0, st, v, p.p, eps.p, W,
                               stats.p, g.p, acc.p, small.p);
        });
        hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(64), 0, st, v, p.p, eps.p, small.p, stats.p, acc.p, g.p, loss.p, extra_loss, tick,
                           lr_t, lr);
    }
};

enum class IsoKind { none, gene, gene_isoform, joint };  // what polee_regression::iso holds

// What a step of fit() with the device RNG tells the passes; the default is an evaluation (polee_regression_eval, the debug hooks,
// steps with supplied noise).
struct RegStep {
    bool tick_in_finish = false;  // reg_finish_kernel advances the device clock
    bool x_drawn = false;         // reg_draw_kernel has written x: reg_data_pass skips reg_sample_x_kernel
    bool update_latent = false;   // reg_latent_kernel also applies Adam to a latent design
};

}  // namespace polee

using namespace polee;

struct polee_regression {
    polee_ctx *ctx = nullptr;
    polee_approx *ap = nullptr;
    float lr = 2e-3f;
    int64_t step = 0;  // ADAM steps taken
    RegBlock main;     // the model of polee_regression_create
    RegBlock iso;      // the second block, of the kind below (empty: none)
    IsoKind kind = IsoKind::none;
    DevBuf<float> d_design, d_W, d_ss, d_x, d_glik, d_lp, d_lse, d_lse_acc, d_lr, d_trace;
    DevBuf<uint32_t> d_tick;
    DevBuf<uint64_t> d_seed;
    hipGraphExec_t graph = nullptr;  // one step (device RNG), replayed by polee_regression_fit
    void drop_graph()
    {
        if (graph) (void)hipGraphExecDestroy(graph);
        graph = nullptr;
    }
    bool lse_valid = false;  // d_lse holds the log-sum-exp of a nearby qx_loc (shift of the multi-block kernel)
    DevBuf<float> d_lik_loc, d_lik_scale;  // point estimates + their scale: the Normal likelihood variant
    // gene-level models: the likelihood handle over nt transcripts; d_xi: x_isoform [S][nt], then d lp / d x_isoform
    polee_approx *gene_ap = nullptr;
    int32_t nt = 0;
    DevBuf<float> d_xi;
    // gene-isoform model (RNASeqGeneIsoformLinearRegression, models/polee_regression.py:656-877): iso is a regression of its own
    // over the transcripts -- horseshoe+ coefficients over the isoform design, x_isoform_bias ~ Normal(0, 2), x_isoform_scale ~
    // InverseGamma(0.001, 0.001) -- a view with deg = 0 and no tail
    DevBuf<float> d_idesign;
    // joint model (RNASeqJointLinearRegression): iso.v = the splice-feature block (iso.v.n features), the transcripts' part its
    // tail; the feature matrix both ways
    DevBuf<int32_t> d_tptr, d_tfeat, d_pptr, d_ptrans;
    DevBuf<float> d_mu, d_resid, d_hinges;
    std::vector<float> h_hinges;  // (kept from create: the joint model's weights follow the sampled bias)
    float bandwidth = 1.0f;
    polee_comm *comm = nullptr;  // samples sharded over ranks: one all-reduce of main.stats per step
    // classify (models/polee_regression.py:342-413): the design matrix is replaced per step (polee_regression_set_design), every
    // evaluation also leaves d loss / d design in d_dF, and Adam only moves the flat parameters [train_lo, train_hi)
    bool want_dgrad = false;
    DevBuf<float> d_dF;  // [REG_SLOTS][S][F]
    // latent design (polee_regression_set_latent_design; RNASeqPCA, models/polee_pca.py:14-92): d_design is the parameter z with its own
    // Adam moments; every evaluation leaves d loss / dz (prior term included) in d_gz and fit() trains z on the device
    bool latent = false;
    float prior_scale = 1.0f;
    DevBuf<float> d_zm, d_zv, d_gz;  // [S][F]
    int64_t train_lo = 0, train_hi = -1;  // (-1: all of them)
};

namespace {

// data pass for the noise in the blocks' eps: main.stats (this rank's samples) and the gradients of qx_*
polee_status reg_data_pass(polee_regression *r, const RegStep &step)
{
    polee_ctx *ctx = r->ctx;
    const RegBlock &mb = r->main, &ib = r->iso;
    const RegView &v = mb.v;
    hipStream_t st = ctx->stream;
    const int64_t sn = (int64_t)v.S * v.n;
    if (!v.point) {
        if (r->lse_valid) {
            hipLaunchKernelGGL(reg_lse_accum_kernel, dim3((unsigned)ceil_div(v.n, 4096), v.S), dim3(256), 0, st, v, mb.p.p, r->d_lse.p,
                               r->d_lse_acc.p);
            hipLaunchKernelGGL(reg_lse_finish_kernel, dim3((unsigned)ceil_div(v.S, 64)), dim3(64), 0, st, v.S, r->d_lse.p, r->d_lse_acc.p);
        } else
            hipLaunchKernelGGL(reg_lse_kernel, dim3(v.S), dim3(1024), 0, st, v, mb.p.p, r->d_lse.p);
        r->lse_valid = true;
        if (!step.x_drawn)
            hipLaunchKernelGGL(reg_sample_x_kernel, dim3((unsigned)ceil_div(sn, 256)), dim3(256), 0, st, v, mb.p.p, mb.eps.p, r->d_x.p);
        POLEE_KERNEL_CHECK(ctx);
        if (r->gene_ap) {
            const dim3 grid((unsigned)ceil_div((int64_t)v.S * r->nt, 256));
            if (r->kind == IsoKind::gene_isoform)
                hipLaunchKernelGGL(reg_sample_x_kernel, grid, dim3(256), 0, st, ib.v, ib.p.p, ib.eps.p, r->d_xi.p);
            else  // the block's tail: all of it (gene), or what follows the splice view (joint)
                hipLaunchKernelGGL(reg_iso_sample_kernel, grid, dim3(256), 0, st, v.S, r->nt, ib.p.p + ib.view_params(),
                                   ib.eps.p + ib.view_noise(), r->d_xi.p);
            POLEE_KERNEL_CHECK(ctx);
            POLEE_TRY(approx_gene_logprob_device(r->gene_ap, r->d_x.p, r->d_xi.p, r->d_lp.p, r->d_glik.p));
        } else if (r->d_lik_loc.p) {
            hipLaunchKernelGGL(reg_normal_lik_kernel, dim3(v.S), dim3(1024), 0, st, v.n, r->d_x.p, r->d_lik_loc.p, r->d_lik_scale.p, r->d_lp.p,
                               r->d_glik.p);
            POLEE_KERNEL_CHECK(ctx);
        } else if (r->ap)
            POLEE_TRY(polee_approx_logprob_device(r->ap, r->d_x.p, r->d_lp.p, r->d_glik.p));
    }
    // (the loss slots of stats, acc and small are zero here: reg_finish_kernel clears what it reads)
    const float *lp = (!v.point && (r->ap || r->d_lik_loc.p || r->gene_ap)) ? r->d_lp.p : nullptr, *none = nullptr;
    reg_dispatch(v, true, [&](auto ft, auto dt) {
        hipLaunchKernelGGL((reg_data_kernel<decltype(ft)::value, decltype(dt)::value>), dim3((unsigned)ceil_div(v.n, REG_BLOCK)), dim3(REG_BLOCK),
                           0, st, v, mb.p.p, mb.eps.p, r->d_design.p, r->d_W.p, r->d_ss.p, r->d_x.p, r->d_glik.p, r->d_lse.p, lp, mb.g.p, mb.stats.p);
    });
    // (d_xi now holds d lp / d x_isoform)
    if (r->kind == IsoKind::joint) {  // the splice block's predictor, the transcripts, back to the features
        const RegView &vs = ib.v;
        const int P = vs.n;
        hipLaunchKernelGGL(reg_joint_mean_kernel, dim3((unsigned)ceil_div(P, 128)), dim3(128), 0, st, vs, v.S, ib.p.p, ib.eps.p, r->d_design.p,
                           r->d_mu.p);
        hipLaunchKernelGGL(reg_joint_iso_kernel, dim3((unsigned)ceil_div(r->nt, 256)), dim3(256), 0, st, v.S, r->nt, P, ib.p.p + vs.num_params(),
                           ib.eps.p + vs.num_noise(), r->d_xi.p, r->d_mu.p, r->d_tptr.p, r->d_tfeat.p, ib.g.p + vs.num_params(), r->d_resid.p,
                           mb.loss_slots());
        hipLaunchKernelGGL(reg_joint_agg_kernel, dim3((unsigned)ceil_div(P, 128)), dim3(128), 0, st, v.S, r->nt, P, vs.F, r->d_resid.p,
                           r->d_design.p, r->d_pptr.p, r->d_ptrans.p, ib.stats.p);
    } else if (r->kind == IsoKind::gene_isoform)  // the isoform block's own data pass
        hipLaunchKernelGGL((reg_data_kernel<0, 0>), dim3((unsigned)ceil_div(r->nt, REG_BLOCK)), dim3(REG_BLOCK), 0, st, ib.v, ib.p.p, ib.eps.p,
                           r->d_idesign.p, none, none, none, r->d_xi.p, none, none, ib.g.p, ib.stats.p);
    else if (r->kind == IsoKind::gene)
        hipLaunchKernelGGL(reg_iso_grad_kernel, dim3((unsigned)ceil_div(r->nt, 256)), dim3(256), 0, st, v.S, r->nt, ib.p.p, ib.eps.p, r->d_xi.p,
                           ib.g.p, mb.loss_slots());
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// prior pass: stats (summed over ranks) -> loss and the gradients of everything the ranks share: the second block if it has
// columns (its loss joins the model's), then the main one
polee_status reg_prior_pass(polee_regression *r, const RegStep &step)
{
    const bool second = r->iso.has_cols();
    if (second) r->iso.launch_prior(r->ctx->stream, nullptr, nullptr, nullptr, nullptr, 0.0f);
    r->main.launch_prior(r->ctx->stream, r->d_W.p, second ? r->iso.loss.p : nullptr, step.tick_in_finish ? r->d_tick.p : nullptr, r->d_lr.p,
                         r->lr);
    POLEE_KERNEL_CHECK(r->ctx);
    return POLEE_OK;
}

// loss and gradient at the current parameters for the noise in the blocks' eps
polee_status reg_eval_device(polee_regression *r, const RegStep &step = RegStep{})
{
    polee_ctx *ctx = r->ctx;
    const RegBlock &mb = r->main;
    const RegView &v = mb.v;
    POLEE_TRY(reg_data_pass(r, step));
    if (r->want_dgrad) {
        if (!r->latent)  // (a latent handle's copies are zero here: reg_latent_kernel clears what it reads)
            POLEE_HIP_TRY(ctx, hipMemsetAsync(r->d_dF.p, 0, sizeof(float) * (size_t)REG_SLOTS * v.S * v.F, ctx->stream));
        hipLaunchKernelGGL(reg_design_grad_kernel, dim3((unsigned)ceil_div(v.n, REG_BLOCK)), dim3(REG_BLOCK), 0, ctx->stream, v, mb.p.p,
                           mb.eps.p, r->d_design.p, r->d_W.p, r->d_ss.p, r->d_x.p, r->d_dF.p);
        POLEE_KERNEL_CHECK(ctx);
    }
    if (r->comm && r->comm->nranks > 1) POLEE_TRY(comm_allreduce_device(r->comm, mb.stats.p, (size_t)mb.num_stats(), false));
    POLEE_TRY(reg_prior_pass(r, step));
    if (r->latent) {
        const float sg = r->prior_scale;
        hipLaunchKernelGGL(reg_latent_kernel, dim3(1), dim3(256), 0, ctx->stream, v.S * v.F, r->d_dF.p, r->d_design.p, r->d_zm.p, r->d_zv.p,
                           r->d_gz.p, 1.0f / (sg * sg), logf(sg) + HALF_LOG2PI, r->d_lr.p, mb.loss.p, step.update_latent ? 1 : 0);
        POLEE_KERNEL_CHECK(ctx);
    }
    return POLEE_OK;
}

// The latents every rank shares are drawn from (seed, step) alone, so that replicas stay identical; the noise of x belongs to a
// rank's own samples and is salted with the rank.
uint64_t rank_salt(const polee_regression *r) { return REG_RANK_SALT * (uint64_t)(r->comm ? r->comm->rank + 1 : 1); }

// seed / step: immediates, or (device_clock) the fit's seed and the clock's value + tick_ahead
void reg_launch_noise(polee_regression *r, int64_t count, uint64_t seed, uint32_t step, bool device_clock, uint64_t salt, float *eps,
                      uint32_t tick_ahead = 0u)
{
    hipLaunchKernelGGL(reg_noise_kernel, dim3((unsigned)ceil_div(ceil_div(count, 4), 256)), dim3(256), 0, r->ctx->stream, count, seed, step,
                       device_clock ? r->d_seed.p : nullptr, device_clock ? r->d_tick.p : nullptr, salt, eps, tick_ahead);
}

polee_status reg_fill_noise(polee_regression *r, const float *noise, uint64_t seed, uint32_t step, bool device_clock)
{
    RegBlock &mb = r->main, &ib = r->iso;
    const int64_t ne = mb.num_noise(), shared = mb.v.e_x(), own = ne - shared;
    if (noise) {
        POLEE_TRY(mb.eps.upload(r->ctx, noise, (size_t)ne));
        if (r->gene_ap) POLEE_TRY(ib.eps.upload(r->ctx, noise + ne, (size_t)ib.num_noise()));
        return POLEE_OK;
    }
    reg_launch_noise(r, shared, seed, step, device_clock, 0, mb.eps.p);
    reg_launch_noise(r, own, seed, step, device_clock, rank_salt(r), mb.eps.p + shared);
    if (r->gene_ap) reg_launch_noise(r, ib.num_noise(), seed, step, device_clock, rank_salt(r) ^ REG_ISO_SALT, ib.eps.p);
    POLEE_KERNEL_CHECK(r->ctx);
    return POLEE_OK;
}

// one step of fit() on the device clock: tick, draw, loss + gradient, Adam (+ the loss into the trace)
polee_status reg_enqueue_step(polee_regression *r, const float *noise, bool want_trace)
{
    polee_ctx *ctx = r->ctx;
    const RegBlock &mb = r->main, &ib = r->iso;
    const RegView &v = mb.v;
    RegStep step;
    step.update_latent = r->latent;
    if (noise) {  // the caller's noise: uploaded; the clock ticks in its own launch
        hipLaunchKernelGGL(reg_tick_kernel, dim3(1), dim3(1), 0, ctx->stream, r->d_tick.p, r->d_lr.p, r->lr);
        POLEE_TRY(reg_fill_noise(r, noise, 0, 0, true));
    } else {
        // device RNG: one launch draws every latent of the step number the clock is ABOUT to show and x with it; the clock is
        // advanced by reg_finish_kernel (in front of Adam, behind everything that reads the noise)
        const int64_t shared = v.e_x(), own = v.num_noise() - shared;
        step.tick_in_finish = true;
        step.x_drawn = !v.point && own == (int64_t)v.S * v.n;
        hipLaunchKernelGGL(reg_draw_kernel, dim3((unsigned)ceil_div((shared + 3) / 4 + (own + 3) / 4, 256)), dim3(256), 0, ctx->stream, v, shared,
                           own, r->d_seed.p, r->d_tick.p, rank_salt(r), mb.p.p, mb.eps.p, step.x_drawn ? r->d_x.p : nullptr);
        if (r->gene_ap) reg_launch_noise(r, ib.num_noise(), 0, 0u, true, rank_salt(r) ^ REG_ISO_SALT, ib.eps.p, 1u);
    }
    POLEE_TRY(reg_eval_device(r, step));
    const int64_t lo = r->train_hi < 0 ? 0 : r->train_lo, cnt = r->train_hi < 0 ? v.num_params() : r->train_hi - r->train_lo;
    hipLaunchKernelGGL(reg_adam_kernel, dim3((unsigned)std::max<int64_t>(ceil_div(cnt, 256), 1)), dim3(256), 0, ctx->stream, cnt, mb.p.p + lo,
                       mb.g.p + lo, mb.m.p + lo, mb.vv.p + lo, r->d_lr.p, mb.loss.p, want_trace ? r->d_trace.p : nullptr, r->d_tick.p);
    if (r->gene_ap)
        hipLaunchKernelGGL(reg_adam_kernel, dim3((unsigned)ceil_div(ib.num_params(), 256)), dim3(256), 0, ctx->stream, ib.num_params(), ib.p.p,
                           ib.g.p, ib.m.p, ib.vv.p, r->d_lr.p, mb.loss.p, (float *)nullptr, r->d_tick.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// column means over the S rows of x [S][n]
std::vector<double> column_means(const float *x, int S, int n)
{
    std::vector<double> mean((size_t)n, 0.0);
    for (int s = 0; s < S; ++s)
        for (int j = 0; j < n; ++j) mean[(size_t)j] += x[(size_t)s * n + j];
    for (auto &m : mean) m /= S;
    return mean;
}

// Initial values of the horseshoe part of a view and of its bias and x_scale rows (models/polee_regression.py:49-119, :740-775,
// :925-1010) into p (zeros): every loc 0 and every softplus scale -1, but qw_softplus_scale = w_s, the bias loc = bias_loc
// (null: 0) and the x_scale loc = xs_loc (a view without x_scale keeps both of its rows at 0)
void init_view_params(const RegView &v, std::vector<float> &p, float w_s, const double *bias_loc, float xs_loc)
{
    const int64_t Fn = v.Fn();
    p[1] = p[3] = -1.0f;
    for (int a = 1; a < 8; a += 2) std::fill_n(p.begin() + v.o_cols() + a * Fn, Fn, -1.0f);
    std::fill_n(p.begin() + v.o_cols() + 9 * Fn, Fn, w_s);
    for (int j = 0; j < v.n; ++j) {
        p[(size_t)(v.o_bias_loc() + j)] = bias_loc ? (float)bias_loc[j] : 0.0f;
        p[(size_t)(v.o_bias_s() + j)] = -1.0f;
        p[(size_t)(v.o_xs_loc() + j)] = v.no_xs ? 0.0f : xs_loc;
        p[(size_t)(v.o_xs_s() + j)] = v.no_xs ? 0.0f : -1.0f;
    }
}

// What the three gene-level likelihoods share.  First their checks of the handle and of ap (nt: its transcripts) ...
polee_status gene_likelihood_check(polee_regression *r, polee_approx *ap, int32_t *nt)
{
    polee_ctx *ctx = r->ctx;
    int32_t aS;
    approx_dims(ap, &aS, nt);
    if (approx_ctx(ap) != ctx || aS != r->main.v.S)
        return fail(ctx, POLEE_ERR_BAD_ARG, "the approximation handle holds %d samples, the model %d", aS, r->main.v.S);
    if (r->main.v.point) return fail(ctx, POLEE_ERR_UNSUPPORTED, "the gene-level model is built without point estimates only");
    if (r->latent) return fail(ctx, POLEE_ERR_UNSUPPORTED, "a latent design belongs to the transcript-level model only");
    if (r->comm && r->comm->nranks > 1) return fail(ctx, POLEE_ERR_UNSUPPORTED, "the gene-level model is not sharded over ranks");
    return POLEE_OK;
}
// ... then, with the second block built, their last steps that can fail -- x_isoform's buffer, and the caller's approximation
// handle learns the genes (the model's features) ...
polee_status gene_likelihood_prepare(polee_regression *r, polee_approx *ap, const int32_t *gene_of, int32_t nt, DevBuf<float> &xi)
{
    POLEE_TRY(xi.alloc(r->ctx, (size_t)r->main.v.S * nt));
    return approx_set_genes(ap, gene_of, r->main.v.n);
}
// ... and only then the handle changes: nothing here can fail.
void gene_likelihood_attach(polee_regression *r, polee_approx *ap, int32_t nt, IsoKind kind, RegBlock &blk, DevBuf<float> &xi)
{
    r->drop_graph();
    r->gene_ap = ap;
    r->nt = nt;
    r->ap = nullptr;
    r->kind = kind;
    r->iso.take(blk);
    r->d_xi.take(xi);
}

}  // namespace

extern "C" {

polee_status polee_regression_create(polee_ctx *ctx, polee_approx *ap, int32_t S, int32_t F, int32_t n,
                                     const float *design, const float *x_init, const float *x_init_mean,
                                     const float *sample_scales, const float *hinges, int32_t degree, float bandwidth, float x_bias_loc0,
                                     float x_bias_scale0, int use_distortion, float scale_penalty,
                                     int use_point_estimates, polee_regression **out)
{
    return ctx_entry(ctx, "polee_regression_create", [&]() -> polee_status {
        if (!out || !design || !x_init || !sample_scales || S < 1 || F < 1 || n < 1 || degree < 1)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_create: bad argument");
        if (F > REG_MAXF || degree > REG_MAXDEG)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "at most %d factors and %d hinges (got %d, %d)", REG_MAXF, REG_MAXDEG, F, degree);
        if (!(bandwidth > 0.0f) || !(x_bias_scale0 > 0.0f) || (!use_point_estimates && !(scale_penalty > 0.0f)))
            return fail(ctx, POLEE_ERR_BAD_ARG, "bandwidth, x_bias_scale0 and scale_penalty must be positive");
        if (ap) {
            int32_t aS, an;
            approx_dims(ap, &aS, &an);
            if (approx_ctx(ap) != ctx || aS != S || an != n)
                return fail(ctx, POLEE_ERR_BAD_ARG, "the approximation handle holds %d x %d, the model %d x %d", aS, an, S, n);
        }
        // (the handle is destroyed on every early return and when something below throws)
        std::unique_ptr<polee_regression, void (*)(polee_regression *)> handle(new polee_regression(), polee_regression_destroy);
        polee_regression *r = handle.get();
        r->ctx = ctx;
        ctx_retain(ctx);
        r->ap = use_point_estimates ? nullptr : ap;
        const RegView v{S, F, n, degree, use_distortion ? 1 : 0, use_point_estimates ? 1 : 0, x_bias_loc0, x_bias_scale0,
                        use_point_estimates ? 1.0f : scale_penalty};
        const size_t sn = (size_t)S * n;
        // initial values (models/polee_regression.py:49-119); x_init_mean: the column means over ALL samples when this handle
        // holds a shard of them
        const std::vector<double> mean = x_init_mean ? std::vector<double>(x_init_mean, x_init_mean + n) : column_means(x_init, S, n);
        std::vector<float> p((size_t)v.num_params(), 0.0f);
        init_view_params(v, p, 0.0f, mean.data(), -0.5f);
        for (int d = 0; d < degree; ++d) p[(size_t)(v.o_conc() + d)] = p[(size_t)(v.o_scc() + d)] = 1.0f;
        std::copy_n(x_init, sn, p.begin() + v.o_qx_loc());
        std::fill_n(p.begin() + v.o_qx_s(), sn, -1.0f);
        // hinges (choose_knots, src/polee.py:69-76) and kernel-regression weights (:36-47)
        std::vector<double> hg((size_t)degree);
        if (hinges)
            for (int d = 0; d < degree; ++d) hg[(size_t)d] = hinges[d];
        else {
            const double lo = *std::min_element(mean.begin(), mean.end()), hi = *std::max_element(mean.begin(), mean.end());
            const double step = (hi - lo) / (degree + 1);
            for (int d = 0; d < degree; ++d) hg[(size_t)d] = lo + (d + 1) * step;
        }
        r->h_hinges.assign(hg.begin(), hg.end());
        r->bandwidth = bandwidth;
        std::vector<float> W((size_t)degree * n);
        for (int j = 0; j < n; ++j) {
            double tot = 0.0, col[REG_MAXDEG];
            for (int d = 0; d < degree; ++d) {
                const double u = ((double)(float)mean[(size_t)j] - hg[(size_t)d]) / bandwidth;
                col[d] = std::min(std::max(std::exp(-u * u), 1e-10), 1.0);
                tot += col[d];
            }
            for (int d = 0; d < degree; ++d) W[(size_t)d * n + j] = (float)(col[d] / tot);
        }
        POLEE_TRY(r->main.init(ctx, v, 0, 0, p));
        POLEE_TRY(r->d_W.upload(ctx, W));
        POLEE_TRY(r->d_design.upload(ctx, design, (size_t)S * F));
        POLEE_TRY(r->d_ss.upload(ctx, sample_scales, (size_t)S));
        for (DevBuf<float> *b : {&r->d_x, &r->d_glik}) POLEE_TRY(b->alloc(ctx, sn));
        for (DevBuf<float> *b : {&r->d_lp, &r->d_lse, &r->d_lse_acc}) POLEE_TRY(b->alloc(ctx, (size_t)S));
        POLEE_TRY(r->d_lr.alloc(ctx, 1));
        POLEE_TRY(r->d_tick.alloc(ctx, 2));
        POLEE_TRY(r->d_seed.alloc(ctx, 1));
        for (DevBuf<float> *b : {&r->d_glik, &r->d_lse, &r->d_lse_acc}) POLEE_TRY(reg_zero(ctx, *b));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *out = handle.release();
        return POLEE_OK;
    });
}

void polee_regression_destroy(polee_regression *r)
{
    if (!r) return;
    polee_ctx *ctx = r->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    polee_comm_destroy(r->comm);
    r->drop_graph();
    delete r;
    ctx_release(ctx);
}

int64_t polee_regression_num_params(const polee_regression *r) { return r ? r->main.num_params() : 0; }
int64_t polee_regression_num_noise(const polee_regression *r) { return r ? r->main.num_noise() + r->iso.num_noise() : 0; }
int64_t polee_regression_num_isoform_params(const polee_regression *r) { return r ? r->iso.num_params() : 0; }
int64_t polee_debug_regression_num_stats(const polee_regression *r) { return r ? r->main.num_stats() : 0; }

polee_status polee_regression_get_params(polee_regression *r, float *params)
{
    return entry(r, "polee_regression_get_params", [&](polee_ctx *ctx) -> polee_status {
        if (!params) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_get_params: null argument");
        return r->main.p.download(ctx, params, (size_t)r->main.num_params());
    });
}

polee_status polee_regression_set_params(polee_regression *r, const float *params)
{
    return entry(r, "polee_regression_set_params", [&](polee_ctx *ctx) -> polee_status {
        if (!params) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_params: null argument");
        r->lse_valid = false;
        return r->main.p.upload(ctx, params, (size_t)r->main.num_params());
    });
}

polee_status polee_regression_weights(polee_regression *r, float *weights)
{
    return entry(r, "polee_regression_weights", [&](polee_ctx *ctx) -> polee_status {
        if (!weights) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_weights: null argument");
        return r->d_W.download(ctx, weights, (size_t)r->main.v.deg * r->main.v.n);
    });
}

polee_status polee_regression_set_normal_likelihood(polee_regression *r, const float *loc, const float *scale)
{
    return entry(r, "polee_regression_set_normal_likelihood", [&](polee_ctx *ctx) -> polee_status {
        if (!loc || !scale) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_normal_likelihood: null argument");
        if (r->main.v.point) return fail(ctx, POLEE_ERR_BAD_ARG, "a model with point estimates has no likelihood term");
        const size_t sn = (size_t)r->main.v.S * r->main.v.n;
        for (size_t i = 0; i < sn; ++i)
            if (!(scale[i] > 0.0f)) return fail(ctx, POLEE_ERR_BAD_ARG, "scale[%zu] = %g is not positive", i, (double)scale[i]);
        r->drop_graph();
        POLEE_TRY(r->d_lik_loc.upload(ctx, loc, sn));
        return r->d_lik_scale.upload(ctx, scale, sn);
    });
}

polee_status polee_regression_set_gene_likelihood(polee_regression *r, polee_approx *ap, const int32_t *gene_of,
                                                  const float *x_isoform_init)
{
    return entry(r, "polee_regression_set_gene_likelihood", [&](polee_ctx *ctx) -> polee_status {
        if (!ap || !gene_of || !x_isoform_init) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_gene_likelihood: null argument");
        int32_t nt;
        POLEE_TRY(gene_likelihood_check(r, ap, &nt));
        const int S = r->main.v.S;
        const size_t snt = (size_t)S * nt;
        // the block is all tail: mean loc / s [nt], x_isoform loc / s [S][nt]; every s = -2 (models/polee_regression.py:573-577)
        std::vector<float> ip(2 * (size_t)nt + 2 * snt, -2.0f);
        const std::vector<double> mean = column_means(x_isoform_init, S, nt);
        for (int i = 0; i < nt; ++i) ip[(size_t)i] = (float)mean[(size_t)i];
        std::copy_n(x_isoform_init, snt, ip.begin() + 2 * (size_t)nt);
        RegBlock blk;
        DevBuf<float> xi;
        POLEE_TRY(blk.init(ctx, RegView{}, (int64_t)ip.size(), (int64_t)(nt + snt), ip));
        POLEE_TRY(gene_likelihood_prepare(r, ap, gene_of, nt, xi));
        gene_likelihood_attach(r, ap, nt, IsoKind::gene, blk, xi);
        return POLEE_OK;
    });
}

polee_status polee_regression_set_gene_isoform_likelihood(polee_regression *r, polee_approx *ap, const int32_t *gene_of,
                                                          const float *x_isoform_init, const float *design_isoform,
                                                          int32_t num_isoform_factors)
{
    return entry(r, "polee_regression_set_gene_isoform_likelihood", [&](polee_ctx *ctx) -> polee_status {
        if (!ap || !gene_of || !x_isoform_init || !design_isoform) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_gene_isoform_likelihood: null argument");
        const int S = r->main.v.S, Fi = num_isoform_factors;
        int32_t nt;
        if (Fi < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "at least one isoform factor (got %d)", Fi);
        if (Fi > REG_MAXF) return fail(ctx, POLEE_ERR_UNSUPPORTED, "1..%d isoform factors (got %d)", REG_MAXF, Fi);
        POLEE_TRY(gene_likelihood_check(r, ap, &nt));
        // the isoform regression: Fi factors over nt columns, no hinges, bias ~ Normal(0, 2), x_scale ~ InverseGamma(0.001, 0.001);
        // initial values (models/polee_regression.py:740-775)
        RegView vi{S, Fi, nt, 0, 0, 0, 0.0f, 2.0f, 1.0f};
        vi.fixed_ab = 0.001f;
        const size_t snt = (size_t)S * nt;
        std::vector<float> p((size_t)vi.num_params(), 0.0f);
        init_view_params(vi, p, -1.0f, column_means(x_isoform_init, S, nt).data(), 1.0f);
        std::copy_n(x_isoform_init, snt, p.begin() + vi.o_qx_loc());
        std::fill_n(p.begin() + vi.o_qx_s(), snt, -2.0f);
        RegBlock blk;
        DevBuf<float> idesign, xi;
        POLEE_TRY(blk.init(ctx, vi, 0, 0, p));
        POLEE_TRY(idesign.upload(ctx, design_isoform, (size_t)S * Fi));
        POLEE_TRY(gene_likelihood_prepare(r, ap, gene_of, nt, xi));
        gene_likelihood_attach(r, ap, nt, IsoKind::gene_isoform, blk, xi);
        r->d_idesign.take(idesign);
        return POLEE_OK;
    });
}

polee_status polee_regression_set_joint_likelihood(polee_regression *r, polee_approx *ap, const int32_t *gene_of,
                                                   const float *x_isoform_init, int32_t num_splice_features,
                                                   const int32_t *pair_transcript, const int32_t *pair_feature, int64_t num_pairs)
{
    return entry(r, "polee_regression_set_joint_likelihood", [&](polee_ctx *ctx) -> polee_status {
        if (!ap || !gene_of || !x_isoform_init || !pair_transcript || !pair_feature) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_joint_likelihood: null argument");
        RegView &v = r->main.v;
        const int S = v.S, P = num_splice_features;
        int32_t nt;
        if (P < 1 || num_pairs < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "bad splice-feature matrix");
        if (v.use_distortion)
            return fail(ctx, POLEE_ERR_BAD_ARG, "the joint model has no distortion term: create the gene block with use_distortion = 0");
        POLEE_TRY(gene_likelihood_check(r, ap, &nt));
        for (int64_t q = 0; q < num_pairs; ++q)
            if (pair_transcript[q] < 0 || pair_transcript[q] >= nt || pair_feature[q] < 0 || pair_feature[q] >= P)
                return fail(ctx, POLEE_ERR_BAD_ARG, "splice-feature pair %lld out of range", (long long)q);
        // the feature matrix both ways (CSR by transcript, CSR by feature); without pairs the index arrays still have to exist
        const size_t np = (size_t)std::max<int64_t>(num_pairs, 1);
        std::vector<int32_t> tptr((size_t)nt + 1, 0), tfeat(np, 0), pptr((size_t)P + 1, 0), ptrans(np, 0);
        for (int64_t q = 0; q < num_pairs; ++q) {
            ++tptr[(size_t)pair_transcript[q] + 1];
            ++pptr[(size_t)pair_feature[q] + 1];
        }
        for (int i = 0; i < nt; ++i) tptr[(size_t)i + 1] += tptr[(size_t)i];
        for (int i = 0; i < P; ++i) pptr[(size_t)i + 1] += pptr[(size_t)i];
        {
            std::vector<int32_t> ct(tptr.begin(), tptr.end() - 1), cp(pptr.begin(), pptr.end() - 1);
            for (int64_t q = 0; q < num_pairs; ++q) {
                tfeat[(size_t)ct[(size_t)pair_transcript[q]]++] = pair_feature[q];
                ptrans[(size_t)cp[(size_t)pair_feature[q]]++] = pair_transcript[q];
            }
        }
        // the splice block: P columns, horseshoe, bias ~ Normal(0, 10), no x_scale of its own, qw_splice_softplus_scale = -2 (:1062-1087,
        // surrogates :1172-1203); its tail, the transcripts: qx_iso_scale loc 3 / s -1 (:1004-1005), qx_iso loc / s -3 (:1009-1010)
        RegView vs{0, v.F, P, 0, 0, 0, 0.0f, 10.0f, 1.0f};
        vs.levels = 1;
        vs.no_xs = 1;
        const int64_t PS = vs.num_params(), snt = (int64_t)S * nt, tail = 2 * (int64_t)nt + 2 * snt;
        std::vector<float> p((size_t)(PS + tail), 0.0f);
        init_view_params(vs, p, -2.0f, nullptr, 0.0f);
        std::fill_n(p.begin() + PS, nt, 3.0f);
        std::fill_n(p.begin() + PS + nt, nt, -1.0f);
        std::copy_n(x_isoform_init, snt, p.begin() + PS + 2 * (int64_t)nt);
        std::fill_n(p.begin() + PS + 2 * (int64_t)nt + snt, snt, -3.0f);
        RegBlock blk;
        DevBuf<int32_t> d_tptr, d_tfeat, d_pptr, d_ptrans;
        DevBuf<float> d_mu, d_resid, d_hinges, xi;
        POLEE_TRY(blk.init(ctx, vs, tail, nt + snt, p));
        POLEE_TRY(d_mu.alloc(ctx, (size_t)S * P));
        POLEE_TRY(d_resid.alloc(ctx, (size_t)snt));
        POLEE_TRY(d_tptr.upload(ctx, tptr));
        POLEE_TRY(d_pptr.upload(ctx, pptr));
        POLEE_TRY(d_tfeat.upload(ctx, tfeat));
        POLEE_TRY(d_ptrans.upload(ctx, ptrans));
        POLEE_TRY(d_hinges.upload(ctx, r->h_hinges));
        POLEE_TRY(gene_likelihood_prepare(r, ap, gene_of, nt, xi));
        // the gene block becomes the joint model's: a horseshoe (one local level), weights from the sampled bias, HalfCauchy(0, 10)
        // on the mean-variance coefficients, qw_gene_softplus_scale = -2 (:1009-1041, :936-937), Adam(1e-3) (:1215)
        const std::vector<float> qs((size_t)v.Fn(), -2.0f);
        POLEE_HIP_TRY(ctx, hipMemcpy(r->main.p.p + v.o_cols() + 9 * v.Fn(), qs.data(), sizeof(float) * qs.size(), hipMemcpyHostToDevice));
        gene_likelihood_attach(r, ap, nt, IsoKind::joint, blk, xi);
        r->d_mu.take(d_mu), r->d_resid.take(d_resid), r->d_hinges.take(d_hinges);
        r->d_tptr.take(d_tptr), r->d_tfeat.take(d_tfeat), r->d_pptr.take(d_pptr), r->d_ptrans.take(d_ptrans);
        v.levels = 1;
        v.w_from_bias = 1;
        v.hc_scale = 10.0f;
        v.bandwidth = r->bandwidth;
        v.hinges = r->d_hinges.p;
        r->lr = 1e-3f;
        return POLEE_OK;
    });
}

polee_status polee_regression_set_learning_rate(polee_regression *r, float lr)
{
    return entry(r, "polee_regression_set_learning_rate", [&](polee_ctx *ctx) -> polee_status {
        if (!(lr > 0.0f)) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_learning_rate: bad learning rate");
        r->lr = lr;
        r->drop_graph();  // (the step size is an argument of the captured tick kernel)
        return POLEE_OK;
    });
}

polee_status polee_regression_get_isoform_params(polee_regression *r, float *params)
{
    return entry(r, "polee_regression_get_isoform_params", [&](polee_ctx *ctx) -> polee_status {
        if (!params) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_get_isoform_params: null argument");
        return r->gene_ap ? r->iso.p.download(ctx, params, (size_t)r->iso.num_params()) : fail(ctx, POLEE_ERR_BAD_ARG, "no isoform block");
    });
}

polee_status polee_regression_set_isoform_params(polee_regression *r, const float *params)
{
    return entry(r, "polee_regression_set_isoform_params", [&](polee_ctx *ctx) -> polee_status {
        if (!params) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_isoform_params: null argument");
        return r->gene_ap ? r->iso.p.upload(ctx, params, (size_t)r->iso.num_params()) : fail(ctx, POLEE_ERR_BAD_ARG, "no isoform block");
    });
}

// gradient of the isoform block left by the last polee_regression_eval
polee_status polee_regression_get_isoform_grad(polee_regression *r, float *grad)
{
    return entry(r, "polee_regression_get_isoform_grad", [&](polee_ctx *ctx) -> polee_status {
        if (!grad) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_get_isoform_grad: null argument");
        return r->gene_ap ? r->iso.g.download(ctx, grad, (size_t)r->iso.num_params()) : fail(ctx, POLEE_ERR_BAD_ARG, "no isoform block");
    });
}

polee_status polee_regression_set_comm(polee_regression *r, polee_comm *comm)
{
    return entry(r, "polee_regression_set_comm", [&](polee_ctx *ctx) -> polee_status {
        if (comm && comm->nranks > 1 && r->gene_ap)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "the gene-level model is not sharded over ranks");
        if (comm && comm->nranks > 1 && r->latent)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "a model with a latent design is not sharded over ranks");
        if (comm && comm->ctx != ctx)
            return fail(ctx, POLEE_ERR_BAD_ARG, "communicator and model belong to different contexts");
        if (comm) ++comm->refs;
        polee_comm_destroy(r->comm);
        r->comm = comm;
        r->drop_graph();
        return POLEE_OK;
    });
}

// test hooks (include/polee_hip_debug.h): the two halves of a step, with the exchange left to the caller
polee_status polee_debug_regression_data_pass(polee_regression *r, const float *noise, float *stats)
{
    return entry(r, "polee_debug_regression_data_pass", [&](polee_ctx *ctx) -> polee_status {
        if (!noise || !stats) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_regression_data_pass: null argument");
        const RegBlock &mb = r->main;
        POLEE_TRY(reg_fill_noise(r, noise, 0, 0, false));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(mb.loss_slots(), 0, sizeof(float) * REG_SLOTS, ctx->stream));
        POLEE_TRY(reg_data_pass(r, RegStep{}));
        POLEE_TRY(mb.stats.download(ctx, stats, (size_t)mb.num_stats()));
        // no finish kernel follows a bare data pass: leave the loss slots clean for the next step
        POLEE_HIP_TRY(ctx, hipMemsetAsync(mb.loss_slots(), 0, sizeof(float) * REG_SLOTS, ctx->stream));
        return POLEE_OK;
    });
}

polee_status polee_debug_regression_prior_pass(polee_regression *r, const float *stats, float *loss, float *grad)
{
    return entry(r, "polee_debug_regression_prior_pass", [&](polee_ctx *ctx) -> polee_status {
        if (!stats || !loss) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_regression_prior_pass: null argument");
        POLEE_TRY(r->main.stats.upload(ctx, stats, (size_t)r->main.num_stats()));
        POLEE_TRY(reg_prior_pass(r, RegStep{}));
        POLEE_TRY(r->main.loss.download(ctx, loss, 1));
        if (grad) POLEE_TRY(r->main.g.download(ctx, grad, (size_t)r->main.num_params()));
        return POLEE_OK;
    });
}

// ---- classify (models/polee_regression.py:342-413) ---------------------------------------------------------------------------------
polee_status polee_regression_set_design(polee_regression *r, const float *design)
{
    return entry(r, "polee_regression_set_design", [&](polee_ctx *ctx) -> polee_status {
        if (!design) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_design: null argument");
        const RegView &v = r->main.v;
        if (r->gene_ap || v.fixed_ab > 0.0f || (r->comm && r->comm->nranks > 1))
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_regression_set_design: the transcript-level model on one GPU only");
        if (!r->want_dgrad) {
            POLEE_TRY(r->d_dF.alloc(ctx, (size_t)REG_SLOTS * v.S * v.F));
            r->want_dgrad = true;
            r->drop_graph();  // (the captured step gains a kernel)
        }
        return r->d_design.upload(ctx, design, (size_t)v.S * v.F);  // (same buffer: a captured step reads the new values)
    });
}

// ---- latent design (RNASeqPCA, models/polee_pca.py:14-92) --------------------------------------------------------------------------
polee_status polee_regression_set_latent_design(polee_regression *r, const float *z0, float prior_scale)
{
    return entry(r, "polee_regression_set_latent_design", [&](polee_ctx *ctx) -> polee_status {
        if (!z0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_latent_design: null argument");
        const RegView &v = r->main.v;
        if (r->gene_ap || v.fixed_ab > 0.0f || (r->comm && r->comm->nranks > 1))
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_regression_set_latent_design: the transcript-level model on one GPU only");
        if (!(prior_scale > 0.0f) || !std::isfinite(prior_scale))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_latent_design: prior_scale = %g is not a positive finite number",
                        (double)prior_scale);
        const size_t SF = (size_t)v.S * v.F;
        r->drop_graph();  // (the captured step loses a memset and gains the update)
        POLEE_TRY(r->d_dF.alloc(ctx, (size_t)REG_SLOTS * SF));
        for (DevBuf<float> *b : {&r->d_zm, &r->d_zv, &r->d_gz}) POLEE_TRY(b->alloc(ctx, SF));
        for (DevBuf<float> *b : {&r->d_dF, &r->d_zm, &r->d_zv, &r->d_gz}) POLEE_TRY(reg_zero(ctx, *b));
        POLEE_TRY(r->d_design.upload(ctx, z0, SF));
        r->want_dgrad = true;
        r->latent = true;
        r->prior_scale = prior_scale;
        return POLEE_OK;
    });
}

polee_status polee_regression_get_design(polee_regression *r, float *design)
{
    return entry(r, "polee_regression_get_design", [&](polee_ctx *ctx) -> polee_status {
        if (!design) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_get_design: null argument");
        return r->d_design.download(ctx, design, (size_t)r->main.v.S * r->main.v.F);
    });
}

polee_status polee_regression_set_trainable(polee_regression *r, int64_t begin, int64_t end)
{
    return entry(r, "polee_regression_set_trainable", [&](polee_ctx *ctx) -> polee_status {
        const int64_t P = r->main.num_params();
        if (begin < 0 || end < begin || end > P)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_set_trainable: [%lld, %lld) of %lld parameters", (long long)begin,
                        (long long)end, (long long)P);
        r->train_lo = begin;
        r->train_hi = end;
        r->drop_graph();
        return POLEE_OK;
    });
}

polee_status polee_regression_design_grad(polee_regression *r, float *grad)
{
    return entry(r, "polee_regression_design_grad", [&](polee_ctx *ctx) -> polee_status {
        if (!grad) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_design_grad: null argument");
        if (!r->want_dgrad) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_design_grad: call polee_regression_set_design first");
        const size_t SF = (size_t)r->main.v.S * r->main.v.F;
        if (r->latent) return r->d_gz.download(ctx, grad, SF);  // (the total, prior term included: reg_latent_kernel)
        std::vector<float> h(SF * REG_SLOTS);
        POLEE_TRY(r->d_dF.download(ctx, h.data(), h.size()));
        for (size_t i = 0; i < SF; ++i) {
            double acc = 0.0;
            for (int c = 0; c < REG_SLOTS; ++c) acc += (double)h[(size_t)c * SF + i];
            grad[i] = (float)acc;
        }
        return POLEE_OK;
    });
}

polee_status polee_regression_eval(polee_regression *r, const float *noise, uint64_t seed, float *loss, float *grad)
{
    return entry(r, "polee_regression_eval", [&](polee_ctx *ctx) -> polee_status {
        if (!loss) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_eval: null argument");
        POLEE_TRY(reg_fill_noise(r, noise, seed, (uint32_t)(r->step + 1), false));
        POLEE_TRY(reg_eval_device(r));
        POLEE_TRY(r->main.loss.download(ctx, loss, 1));
        if (grad) POLEE_TRY(r->main.g.download(ctx, grad, (size_t)r->main.num_params()));
        return POLEE_OK;
    });
}

polee_status polee_regression_fit(polee_regression *r, int32_t niter, uint64_t seed, const float *noise, float *loss_trace)
{
    return entry(r, "polee_regression_fit", [&](polee_ctx *ctx) -> polee_status {
        if (niter < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_regression_fit: null argument");
        if (niter == 0) return POLEE_OK;
        hipStream_t st = ctx->stream;
        const int64_t ne = r->main.num_noise() + r->iso.num_noise();
        if (r->d_trace.n < (size_t)niter) {  // (the trace's address is part of the captured step)
            r->drop_graph();
            POLEE_TRY(r->d_trace.alloc(ctx, std::max<size_t>((size_t)niter, 8192)));
        }
        const uint32_t clock[2] = {(uint32_t)r->step, 0u};
        POLEE_TRY(r->d_tick.upload(ctx, clock, 2));
        POLEE_TRY(r->d_seed.upload(ctx, &seed, 1));
        // Steps with the device RNG are replayed from a hipGraph (about 25 launches per step otherwise bound the step on
        // the host); supplied noise, a multi-rank communicator (RCCL inside a capture) or POLEE_REG_NO_GRAPH=1 enqueue
        // directly.  The first step always runs directly: it computes the exact log-sum-exp the later ones start from.
        const bool use_graph = !noise && !(r->comm && r->comm->nranks > 1) && !std::getenv("POLEE_REG_NO_GRAPH");
        int32_t it = 0;
        if (!use_graph || !r->lse_valid) {
            POLEE_TRY(reg_enqueue_step(r, noise, true));
            it = 1;
        }
        if (use_graph && it < niter && !r->graph) {
            hipGraph_t g = nullptr;
            POLEE_HIP_TRY(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            const polee_status cs = reg_enqueue_step(r, nullptr, true);
            const hipError_t ce = hipStreamEndCapture(st, &g);
            if (cs != POLEE_OK || ce != hipSuccess) {
                if (g) (void)hipGraphDestroy(g);
                return cs != POLEE_OK ? cs : fail(ctx, POLEE_ERR_HIP, "graph capture failed: %s", hipGetErrorString(ce));
            }
            const hipError_t ie = hipGraphInstantiate(&r->graph, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ie != hipSuccess) {
                r->graph = nullptr;
                return fail(ctx, POLEE_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
            }
        }
        for (; it < niter; ++it) {
            if (use_graph)
                POLEE_HIP_TRY(ctx, hipGraphLaunch(r->graph, st));
            else
                POLEE_TRY(reg_enqueue_step(r, noise ? noise + (size_t)it * ne : nullptr, true));
        }
        r->step += niter;
        if (loss_trace) POLEE_TRY(r->d_trace.download(ctx, loss_trace, (size_t)niter));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(st));
        return POLEE_OK;
    });
}

}  // extern "C"

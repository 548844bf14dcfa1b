// What the models trained on fresh posterior draws share (classify.hip, tsne.hip, forest.hip; DESIGN.md sections 3.10, 3.13, 3.14):
// device building blocks templated on KP (the number of output columns padded to 2, 4, 8 or 16) that the models' kernels are thin
// bodies around, and the host plumbing around a draw.  The __global__ entry points, their names and their launch geometry stay with
// the models.  Every sum here has a fixed order and there are no float atomics: the kernels built from these blocks are bitwise
// reproducible, and with the default -ffp-contract=fast the shape of an expression decides what the backend fuses -- change none.
#pragma once
#include "common.hpp"
#include "wave.hpp"  // wave_split_reduce

#include <cmath>
#include <type_traits>

namespace polee {

constexpr int DM_BLOCK = 256;
constexpr int DM_WAVE_J = 128;  // transcripts per chunk of a projection: one wave, two per lane
constexpr int DM_TILE_S = 64;   // samples whose column gradients the gradient accumulation stages in LDS at a time

// lx of one value: the log of a draw, or an uploaded point as it is; BIAS: minus the transcript's bias
template <bool BIAS>
__device__ __forceinline__ float lx_of(float v, int is_log, float b)
{
    if constexpr (BIAS)
        return (is_log ? v : logf(v)) - b;
    else
        return is_log ? v : logf(v);
}

// Chunk projection, one wave per chunk of DM_WAVE_J transcripts (DM_BLOCK / 64 chunks per workgroup, no barrier): the wave keeps its
// chunk of wT [k][n] (and of xb [n] with BIAS) in registers for all S samples; per sample two f32 FMAs per column in the lane, then
// the fixed shuffle tree over the lanes.  part [nchunks][S][k].  The models' extras: abs_part [nchunks] (or null), the chunk's
// sum |w| (classify's L1 term); with ROW_SUM rpart [nchunks][S], the chunk's sum of lx (tsne's row means).
template <int KP, bool BIAS, bool ROW_SUM>
__device__ __forceinline__ void chunk_project(int n, int S, int k, int nchunks, const float *x, int is_log,
                                     const float *wT, const float *xb, float *part,
                                     float *abs_part, float *rpart)
{
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * (DM_BLOCK / 64) + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;  // (wave-uniform)
    const int64_t j0 = (int64_t)chunk * DM_WAVE_J + lane, j1 = j0 + 64;
    const bool a0 = j0 < n, a1 = j1 < n;
    float w0[KP], w1[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        w0[c] = (a0 && c < k) ? wT[(int64_t)c * n + j0] : 0.0f;
        w1[c] = (a1 && c < k) ? wT[(int64_t)c * n + j1] : 0.0f;
    }
    float b0 = 0.0f, b1 = 0.0f;
    if constexpr (BIAS) {
        b0 = a0 ? xb[j0] : 0.0f;
        b1 = a1 ? xb[j1] : 0.0f;
    }
    if (abs_part) {
        float a = 0.0f;
#pragma unroll
        for (int c = 0; c < KP; ++c) a += fabsf(w0[c]) + fabsf(w1[c]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) abs_part[chunk] = a;
    }
    constexpr int PER = 64 / KP;
    const int col = lane / PER;
    const bool writer = (lane % PER) == 0 && col < k;
    for (int s = 0; s < S; ++s) {
        const float *xs = x + (int64_t)s * n;
        const float v0 = a0 ? xs[j0] : 1.0f, v1 = a1 ? xs[j1] : 1.0f;
        const float l0 = a0 ? lx_of<BIAS>(v0, is_log, b0) : 0.0f;
        const float l1 = a1 ? lx_of<BIAS>(v1, is_log, b1) : 0.0f;
        float p[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) p[c] = fmaf(l1, w1[c], l0 * w0[c]);
        wave_split_reduce<KP>(p, lane);
        if constexpr (ROW_SUM) {
            float r = l0 + l1;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) r += __shfl_xor(r, off, 64);
            if (writer) part[((int64_t)chunk * S + s) * k + col] = p[0];
            if (lane == 0) rpart[(int64_t)chunk * S + s] = r;
        } else {
            if (writer) part[((int64_t)chunk * S + s) * k + col] = p[0];
        }
    }
}

// Gradient accumulation of transcript j (one thread per transcript, coalesced over j, every x[s][j] read once):
// acc[c] = sum_s lx[s][j] d[s][c], d [S][k] staged in sd (LDS, DM_TILE_S * KP floats) DM_TILE_S samples at a time and read as
// broadcasts.  With DSUM thread c < KP also returns dsum = sum_s d[s][c] in f64 (classify's bias gradients).
template <int KP, bool BIAS, bool DSUM>
__device__ __forceinline__ void grad_accumulate(int n, int S, int k, const float *x, int is_log, const float *d,
                                       int64_t j, bool active, float xbj, float *sd, float (&acc)[KP], double &dsum)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0f;
    dsum = 0.0;
    for (int s0 = 0; s0 < S; s0 += DM_TILE_S) {
        const int ns = min(DM_TILE_S, S - s0);
        __syncthreads();
        for (int e = tid; e < ns * KP; e += DM_BLOCK) {
            const int s = e / KP, c = e % KP;
            sd[e] = c < k ? d[(int64_t)(s0 + s) * k + c] : 0.0f;
        }
        __syncthreads();
        if constexpr (DSUM)
            if (tid < KP)
                for (int s = 0; s < ns; ++s) dsum += (double)sd[s * KP + tid];
        if (active) {
#pragma unroll 4
            for (int s = 0; s < ns; ++s) {
                const float v = x[(int64_t)(s0 + s) * n + j];
                const float lx = lx_of<BIAS>(v, is_log, xbj);
#pragma unroll
                for (int c = 0; c < KP; ++c) acc[c] = fmaf(lx, sd[s * KP + c], acc[c]);
            }
        }
    }
}

// red[c], c < k: the sum over the chunks of part [nchunks][S][k] for sample s, in f64 in a fixed order: thread (column c = tid % KP,
// stripe q = tid / KP) sums chunks q, q + Q, .., the stripes are folded by a tree.  red: DM_BLOCK doubles of LDS; RED_BUSY: other
// threads may still be reading it.
template <int KP, bool RED_BUSY>
__device__ __forceinline__ void chunk_sum(const float *part, int S, int k, int nchunks, int s, double *red)
{
    constexpr int Q = DM_BLOCK / KP;
    const int tid = threadIdx.x, c = tid % KP, q = tid / KP;
    double a = 0.0;
    if (c < k)
        for (int ch = q; ch < nchunks; ch += Q) a += (double)part[((int64_t)ch * S + s) * k + c];
    if constexpr (RED_BUSY) __syncthreads();
    red[tid] = a;
    __syncthreads();
    for (int o = Q / 2; o >= 1; o >>= 1) {
        if (q < o) red[tid] += red[tid + o * KP];
        __syncthreads();
    }
}

// every thread gets the sum over the workgroup of v, in a fixed order (red: DM_BLOCK doubles of LDS)
__device__ inline double block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = DM_BLOCK / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// Adam in the TF form (tf.optimizers.Adam, tf.train.AdamOptimizer): p -= lr_t m / (sqrt(v) + eps), lr_t = tf_adam_rate() from the
// host.  Updates the moments in place and returns the new p.  (regression_device.hpp's adam_step is another function on purpose.)
__device__ __forceinline__ float tf_adam(float p, float *m, float *v, float g, float lr_t, float b1, float b2, float eps)
{
    const float mn = b1 * *m + (1.0f - b1) * g;
    const float vn = b2 * *v + (1.0f - b2) * g * g;
    *m = mn;
    *v = vn;
    return p - lr_t * mn / (sqrtf(vn) + eps);
}

// out = the mean of an f64 accumulator over ndraws draws
static __global__ void acc_mean_kernel(int64_t count, const double *__restrict__ acc, double ndraws, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = (float)(acc[i] / ndraws);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
inline polee_status launch_acc_mean(polee_ctx *ctx, int64_t count, const double *d_acc, int32_t ndraws, float *d_out)
{
    hipLaunchKernelGGL(acc_mean_kernel, dim3((unsigned)ceil_div(count, DM_BLOCK)), dim3(DM_BLOCK), 0, ctx->stream, count, d_acc,
                       (double)ndraws, d_out);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// the bias-corrected rate of Adam step t
inline double tf_adam_rate(double lr, double b1, double b2, int64_t t)
{
    return lr * std::sqrt(1.0 - std::pow(b2, (double)t)) / (1.0 - std::pow(b1, (double)t));
}

inline int32_t kp_of(int32_t k) { return k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

// f(std::integral_constant<int, KP>) for the KP the kernels are built for
template <class F>
inline polee_status dispatch_kp(int KP, F &&f)
{
    switch (KP) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
    }
}

// the device's wT [k][n] <-> the ABI's w [n][k]
inline void wT_to_abi(const float *wT, int64_t n, int64_t k, float *w)
{
    for (int64_t j = 0; j < n; ++j)
        for (int64_t c = 0; c < k; ++c) w[j * k + c] = wT[c * n + j];
}
inline void abi_to_wT(const float *w, int64_t n, int64_t k, float *wT)
{
    for (int64_t j = 0; j < n; ++j)
        for (int64_t c = 0; c < k; ++c) wT[c * n + j] = w[j * k + c];
}

// the approximation a model draws from: on the model's context, of its n and (S_expected > 0) its S.  who: "polee_<model>"
inline polee_status check_approx(polee_ctx *ctx, const char *who, polee_approx *ap, int32_t n, int32_t S_expected, int32_t *S)
{
    if (!ap) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: null approximation handle", who);
    int32_t an = 0;
    approx_dims(ap, S, &an);
    if (approx_ctx(ap) != ctx) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: the approximation lives on another context", who);
    if (S_expected > 0 && (an != n || *S != S_expected))
        return fail(ctx, POLEE_ERR_BAD_ARG, "%s: the approximation has S = %d, n = %d, the model S = %d, n = %d", who, *S, an, S_expected, n);
    if (an != n) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: the approximation has n = %d, the model n = %d", who, an, n);
    return POLEE_OK;
}

// uploaded points x [rows][n] (log expression): the reference takes log 0 = -inf silently when a TPM is 0 and no pseudocount is given
// (classify.jl:141-147)
inline polee_status check_points(polee_ctx *ctx, const char *who, const float *x, int64_t rows, int32_t n)
{
    if (!x || rows < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: bad argument", who);
    const size_t cnt = (size_t)rows * n;
    for (size_t i = 0; i < cnt; ++i)
        if (!std::isfinite(x[i]))
            return fail(ctx, POLEE_ERR_NONFINITE, "%s: x[%zu][%zu] is not finite (log of a zero point estimate? add a pseudocount)", who,
                        i / n, i % n);
    return POLEE_OK;
}

// The draws of one call.  Draw `index` is made under seed + POLEE_DRAW_STRIDE * index (the index is classify's (t - 1) D + d, tsne's
// t - 1, the plain draw number elsewhere); with z0 its N(0,1) noise is slot `slot` of the array uploaded once before the loop.
struct DrawFeed {
    polee_approx *ap;
    DevBuf<float> &d_z0;
    size_t sk;  // S (n - 1): the noise of one draw
    uint64_t seed;
    bool have_z0 = false;
    DrawFeed(polee_approx *ap_, DevBuf<float> &buf, int32_t S, int32_t n, uint64_t seed_) : ap(ap_), d_z0(buf), sk((size_t)S * (n - 1)), seed(seed_) {}
    polee_status upload(const float *z0, size_t draws)
    {
        have_z0 = z0 != nullptr;
        return z0 ? d_z0.upload(approx_ctx(ap), z0, draws * sk) : POLEE_OK;
    }
    // queues the draw on the context's stream; *x = f32 [S][n] on the device, clipped at 1e-16
    polee_status draw(uint64_t index, size_t slot, const float **x)
    {
        POLEE_TRY(approx_sample_device(ap, have_z0 ? d_z0.p + slot * sk : nullptr, seed + POLEE_DRAW_STRIDE * index));
        *x = approx_draw_buffer(ap);
        return POLEE_OK;
    }
};

// after the last step of a fit call: the clock advances, the loss trace (or nothing) comes back
inline polee_status fit_finish(polee_ctx *ctx, int64_t *t, const DevBuf<float> &d_loss, int32_t niter, float *loss_trace)
{
    *t += niter;
    if (loss_trace) return d_loss.download(ctx, loss_trace, (size_t)niter);
    POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return POLEE_OK;
}

}  // namespace polee

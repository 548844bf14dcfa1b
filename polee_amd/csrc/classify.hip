// `polee model classify` (models/classify.jl, models/polee_classify.py:13-114): multinomial logistic regression on log expression,
// trained on fresh draws from the training samples' fitted approximations at every step, predicting by the mean class probability over
// draws from the testing samples' approximations.  DESIGN.md section 3.10.
//
//   logits[s][c] = sum_j (lx[s][j] - x_bias[j]) w[j][c] + z_bias[c]           lx = log of a draw, or an uploaded point estimate
//   loss         = loss_scale / D  sum_d sum_s CE(labels_s, softmax(logits_s)) + l1 sum |w|
//
// Per draw, on the context's stream, nothing waits for the device:
//   1. approx_sample_device           the draw x [S][n] (approx.hip), clipped at 1e-16 so logf is finite
//   2. classify_logits_kernel         grid over chunks of CL_WAVE_J transcripts, one wave per chunk: the wave keeps its chunk of w and
//                                     x_bias in registers for all S samples; f32 FMAs over the lane's transcripts, then a fixed
//                                     shuffle tree over the lanes; partials [chunks][S][k]
//   3. classify_finish_kernel         one workgroup per sample: the partials summed in f64 in a fixed order, + z_bias, softmax in f64;
//                                     training: dl = (softmax - labels) loss_scale / D and the sample's loss term; prediction:
//                                     probabilities accumulated in f64
//   4. classify_grad_kernel           one thread per transcript, coalesced over j, reads every x[s][j] once; dl staged in LDS
//                                     g_w[c][j] += sum_s (lx - x_bias[j]) dl[s][c];  g_xb[j] -= sum_c w[j][c] sum_s dl[s][c];
//                                     workgroup 0 adds the draw's g_zb and loss
// After the last draw of a step classify_update_kernel adds l1 sign(w), applies Adam (the TF form, as regression.hip) to w, x_bias and
// z_bias and leaves the accumulators at zero; in evaluation mode it hands the same gradients out instead.
// There are no float atomics: every sum has a fixed order, so results are bitwise reproducible.
// Parameters, moments and accumulators share one flat layout: wT [k][n] | x_bias [n] | z_bias [k] (the ABI speaks w [n][k]).
#include "common.hpp"
#include "wave.hpp"  // wave_split_reduce

#include <cmath>

namespace polee {

constexpr int CL_BLOCK = 256;
constexpr int CL_WAVE_J = 128;  // transcripts per chunk of the logits kernel: one wave, two per lane
constexpr int CL_TILE_S = 64;   // samples whose dl the gradient kernel stages in LDS at a time
constexpr uint64_t CL_DRAW_STRIDE = 0x9E3779B97F4A7C15ull;  // draw i uses seed + stride * i (as polee_approx_feature_moments)

// part [nchunks][S][k]; abs_part [nchunks] or null: sum |w| of the chunk (the L1 term of the loss, once per step)
template <int KP>
__global__ __launch_bounds__(CL_BLOCK) void classify_logits_kernel(int n, int S, int k, int nchunks, const float *__restrict__ x,
                                                                  int is_log, const float *__restrict__ P,
                                                                  float *__restrict__ part, float *__restrict__ abs_part)
{
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * (CL_BLOCK / 64) + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;  // (wave-uniform; the kernel has no barrier)
    const int64_t j0 = (int64_t)chunk * CL_WAVE_J + lane, j1 = j0 + 64;
    const bool a0 = j0 < n, a1 = j1 < n;
    const float *xb = P + (int64_t)k * n;
    float w0[KP], w1[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) {
        w0[c] = (a0 && c < k) ? P[(int64_t)c * n + j0] : 0.0f;
        w1[c] = (a1 && c < k) ? P[(int64_t)c * n + j1] : 0.0f;
    }
    const float b0 = a0 ? xb[j0] : 0.0f, b1 = a1 ? xb[j1] : 0.0f;
    if (abs_part) {
        float a = 0.0f;
#pragma unroll
        for (int c = 0; c < KP; ++c) a += fabsf(w0[c]) + fabsf(w1[c]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) abs_part[chunk] = a;
    }
    constexpr int PER = 64 / KP;
    const int cls = lane / PER;
    const bool writer = (lane % PER) == 0 && cls < k;
    for (int s = 0; s < S; ++s) {
        const float *xs = x + (int64_t)s * n;
        const float v0 = a0 ? xs[j0] : 1.0f, v1 = a1 ? xs[j1] : 1.0f;
        const float l0 = a0 ? (is_log ? v0 : logf(v0)) - b0 : 0.0f;
        const float l1 = a1 ? (is_log ? v1 : logf(v1)) - b1 : 0.0f;
        float p[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) p[c] = fmaf(l1, w1[c], l0 * w0[c]);
        wave_split_reduce<KP>(p, lane);
        if (writer) part[((int64_t)chunk * S + s) * k + cls] = p[0];
    }
}

// grid S (+ 1 when abs_part: that workgroup sums the L1 term into lossacc[1]).  mode 0: dl [S][k], loss_s [S]; mode 1: probs [S][k] +=
template <int KP>
__global__ __launch_bounds__(CL_BLOCK) void classify_finish_kernel(int S, int k, int nchunks, const float *__restrict__ part,
                                                                  const float *__restrict__ zb, const float *__restrict__ labels,
                                                                  double scale, int mode, float *__restrict__ dl,
                                                                  double *__restrict__ loss_s, double *__restrict__ probs,
                                                                  const float *__restrict__ abs_part, double l1,
                                                                  double *__restrict__ lossacc)
{
    __shared__ double red[CL_BLOCK];
    const int tid = threadIdx.x, s = blockIdx.x;
    if (s == S) {  // (only launched with abs_part)
        double a = 0.0;
        for (int ch = tid; ch < nchunks; ch += CL_BLOCK) a += (double)abs_part[ch];
        red[tid] = a;
        __syncthreads();
        for (int o = CL_BLOCK / 2; o >= 1; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) lossacc[1] = l1 * red[0];
        return;
    }
    constexpr int Q = CL_BLOCK / KP;
    const int c = tid % KP, q = tid / KP;
    double a = 0.0;
    if (c < k)
        for (int ch = q; ch < nchunks; ch += Q) a += (double)part[((int64_t)ch * S + s) * k + c];
    red[tid] = a;
    __syncthreads();
    for (int o = Q / 2; o >= 1; o >>= 1) {
        if (q < o) red[tid] += red[tid + o * KP];
        __syncthreads();
    }
    if (tid != 0) return;
    // (thread 0 alone: k <= 16 numbers; the logits stay in LDS so that nothing is indexed at run time in registers)
    double mx = -INFINITY;
    for (int i = 0; i < k; ++i) {
        red[i] += (double)zb[i];
        mx = fmax(mx, red[i]);
    }
    double den = 0.0;
    for (int i = 0; i < k; ++i) den += exp(red[i] - mx);
    const double lse = mx + log(den);
    if (mode == 1) {
        for (int i = 0; i < k; ++i) probs[(int64_t)s * k + i] += exp(red[i] - lse);
        return;
    }
    double ce = 0.0;
    for (int i = 0; i < k; ++i) {
        const double y = (double)labels[(int64_t)s * k + i];
        ce += y * (lse - red[i]);
        dl[(int64_t)s * k + i] = (float)((exp(red[i] - lse) - y) * scale);
    }
    loss_s[s] = ce * scale;
}

// G: the accumulators in the parameters' layout.  Workgroup 0 also adds the draw's g_zb and its loss (lossacc[0]).
template <int KP>
__global__ __launch_bounds__(CL_BLOCK) void classify_grad_kernel(int n, int S, int k, const float *__restrict__ x, int is_log,
                                                                const float *__restrict__ P, const float *__restrict__ dl,
                                                                const double *__restrict__ loss_s, float *__restrict__ G,
                                                                double *__restrict__ lossacc)
{
    __shared__ float sdl[CL_TILE_S * KP];
    __shared__ float sds[KP];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * CL_BLOCK + tid;
    const bool active = j < n;
    const int64_t kn = (int64_t)k * n;
    const float xbj = active ? P[kn + j] : 0.0f;
    float acc[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) acc[c] = 0.0f;
    double dsum = 0.0;
    for (int s0 = 0; s0 < S; s0 += CL_TILE_S) {
        const int ns = min(CL_TILE_S, S - s0);
        __syncthreads();
        for (int e = tid; e < ns * KP; e += CL_BLOCK) {
            const int s = e / KP, c = e % KP;
            sdl[e] = c < k ? dl[(int64_t)(s0 + s) * k + c] : 0.0f;
        }
        __syncthreads();
        if (tid < KP)
            for (int s = 0; s < ns; ++s) dsum += (double)sdl[s * KP + tid];
        if (active) {
#pragma unroll 4
            for (int s = 0; s < ns; ++s) {
                const float v = x[(int64_t)(s0 + s) * n + j];
                const float lx = (is_log ? v : logf(v)) - xbj;
#pragma unroll
                for (int c = 0; c < KP; ++c) acc[c] = fmaf(lx, sdl[s * KP + c], acc[c]);
            }
        }
    }
    if (tid < KP) sds[tid] = (float)dsum;
    __syncthreads();
    if (active) {
        float gx = 0.0f;
#pragma unroll
        for (int c = 0; c < KP; ++c)
            if (c < k) {
                G[(int64_t)c * n + j] += acc[c];
                gx = fmaf(P[(int64_t)c * n + j], sds[c], gx);
            }
        G[kn + j] -= gx;
    }
    if (blockIdx.x == 0) {
        if (tid < k) G[kn + n + tid] += sds[tid];
        if (tid == 0) {
            double L = 0.0;
            for (int s = 0; s < S; ++s) L += loss_s[s];
            lossacc[0] += L;
        }
    }
}

// After the last draw of a step.  mode 0: Adam (tf.optimizers.Adam: p -= lr_t m / (sqrt(v) + eps), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
// from the host); mode 1: the gradients go to gout, nothing is updated.  Either way the accumulators are left at zero and
// loss_out[0] = the step's loss.
__global__ void classify_update_kernel(int64_t total, int64_t kn, float *__restrict__ P, float *__restrict__ G, float *__restrict__ M,
                                       float *__restrict__ V, float lr_t, float b1, float b2, float eps, float l1, int mode,
                                       float *__restrict__ gout, double *__restrict__ lossacc, float *__restrict__ loss_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        loss_out[0] = (float)(lossacc[0] + lossacc[1]);
        lossacc[0] = 0.0;
    }
    if (i >= total) return;
    const float p = P[i];
    float g = G[i];
    G[i] = 0.0f;
    if (i < kn) g += l1 * (float)((p > 0.0f) - (p < 0.0f));  // (d|w|/dw with sign(0) = 0, as tf.abs)
    if (mode == 1) {
        gout[i] = g;
        return;
    }
    const float m = b1 * M[i] + (1.0f - b1) * g;
    const float v = b2 * V[i] + (1.0f - b2) * g * g;
    M[i] = m;
    V[i] = v;
    P[i] = p - lr_t * m / (sqrtf(v) + eps);
}

// x_bias <- the column mean over samples of lx (polee_classify.py:52-55, :75)
__global__ void classify_colmean_kernel(int n, int S, const float *__restrict__ x, int is_log, float *__restrict__ xb)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double a = 0.0;
    for (int s = 0; s < S; ++s) {
        const float v = x[(int64_t)s * n + j];
        a += (double)(is_log ? v : logf(v));
    }
    xb[j] = (float)(a / (double)S);
}

__global__ void classify_probs_kernel(int64_t count, const double *__restrict__ acc, double ndraws, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = (float)(acc[i] / ndraws);
}

}  // namespace polee

using namespace polee;

struct polee_classify {
    polee_ctx *ctx = nullptr;
    int32_t n = 0, k = 0, KP = 0, nchunks = 0;
    int64_t kn = 0, total = 0;
    int64_t t = 0;  // Adam steps taken: the step clock, which runs on across fit calls
    polee_classify_opts o;
    DevBuf<float> d_P, d_M, d_V, d_G, d_gout, d_abs, d_loss;
    DevBuf<double> d_lossacc;  // [0] the cross-entropy terms of the step's draws so far, [1] the L1 term
    // per sample count (grown on demand)
    DevBuf<float> d_part, d_dl, d_labels, d_probs_out, d_x, d_z0;
    DevBuf<double> d_loss_s, d_probs;
    int32_t S_cap = 0;
};

namespace {

polee_status check_opts(polee_ctx *ctx, const polee_classify_opts &o)
{
    if (o.draws_per_step < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: draws_per_step must be at least 1");
    if (!(o.learning_rate > 0.0f) || !std::isfinite(o.learning_rate) || !(o.l1_penalty >= 0.0f) || !std::isfinite(o.l1_penalty) ||
        !std::isfinite(o.loss_scale) || !(o.beta1 >= 0.0f && o.beta1 < 1.0f) || !(o.beta2 >= 0.0f && o.beta2 < 1.0f) ||
        !(o.epsilon > 0.0f) || !std::isfinite(o.epsilon))
        return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: an option is out of range");
    return POLEE_OK;
}

polee_status ensure_samples(polee_classify *cl, int32_t S)
{
    polee_ctx *ctx = cl->ctx;
    if (S < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: S < 1");
    const size_t sk = (size_t)S * cl->k;
    POLEE_TRY(cl->d_part.alloc(ctx, (size_t)cl->nchunks * sk));
    POLEE_TRY(cl->d_dl.alloc(ctx, sk));
    POLEE_TRY(cl->d_labels.alloc(ctx, sk));
    POLEE_TRY(cl->d_probs_out.alloc(ctx, sk));
    POLEE_TRY(cl->d_probs.alloc(ctx, sk));
    POLEE_TRY(cl->d_loss_s.alloc(ctx, (size_t)S));
    cl->S_cap = std::max(cl->S_cap, S);
    return POLEE_OK;
}

// TF's gradient softmax - labels only means something for a distribution; the reference's rows are one-hot (classify.jl:298-305)
polee_status upload_labels(polee_classify *cl, const float *labels, int32_t S)
{
    polee_ctx *ctx = cl->ctx;
    for (int32_t s = 0; s < S; ++s) {
        int ones = 0;
        for (int32_t c = 0; c < cl->k; ++c) {
            const float y = labels[(size_t)s * cl->k + c];
            if (y == 1.0f)
                ++ones;
            else if (y != 0.0f)
                ones = -cl->k - 1;
        }
        if (ones != 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: label row %d is not one-hot", s);
    }
    return cl->d_labels.upload(ctx, labels, (size_t)S * cl->k);
}

// the reference takes log 0 = -inf silently when a TPM is 0 and no pseudocount is given (classify.jl:141-147)
polee_status upload_points(polee_classify *cl, const float *x, int32_t S)
{
    polee_ctx *ctx = cl->ctx;
    if (!x || S < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: bad argument");
    const size_t sn = (size_t)S * cl->n;
    for (size_t i = 0; i < sn; ++i)
        if (!std::isfinite(x[i]))
            return fail(ctx, POLEE_ERR_NONFINITE,
                        "polee_classify: x[%zu][%zu] is not finite (log of a zero point estimate? add a pseudocount)", i / cl->n,
                        i % cl->n);
    return cl->d_x.upload(ctx, x, sn);
}

polee_status check_approx(polee_classify *cl, polee_approx *ap, int32_t *S)
{
    polee_ctx *ctx = cl->ctx;
    if (!ap) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: null approximation handle");
    int32_t n = 0;
    approx_dims(ap, S, &n);
    if (approx_ctx(ap) != ctx) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: the approximation lives on another context");
    if (n != cl->n) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify: the approximation has n = %d, the classifier n = %d", n, cl->n);
    return POLEE_OK;
}

// one draw through the kernels.  mode 0: training (dl, loss, gradient accumulation), 1: prediction (probabilities accumulated)
template <int KP>
polee_status draw_pass_t(polee_classify *cl, const float *d_x, int is_log, int32_t S, double scale, bool first, int mode)
{
    polee_ctx *ctx = cl->ctx;
    hipStream_t st = ctx->stream;
    const bool pen = first && mode == 0;
    hipLaunchKernelGGL((classify_logits_kernel<KP>), dim3((unsigned)ceil_div(cl->nchunks, CL_BLOCK / 64)), dim3(CL_BLOCK), 0, st, cl->n, S,
                       cl->k, cl->nchunks, d_x, is_log, (const float *)cl->d_P.p, cl->d_part.p, pen ? cl->d_abs.p : nullptr);
    hipLaunchKernelGGL((classify_finish_kernel<KP>), dim3((unsigned)(S + (pen ? 1 : 0))), dim3(CL_BLOCK), 0, st, S, cl->k, cl->nchunks,
                       (const float *)cl->d_part.p, (const float *)(cl->d_P.p + cl->kn + cl->n), (const float *)cl->d_labels.p, scale,
                       mode, cl->d_dl.p, cl->d_loss_s.p, cl->d_probs.p, (const float *)(pen ? cl->d_abs.p : nullptr),
                       (double)cl->o.l1_penalty, cl->d_lossacc.p);
    if (mode == 0)
        hipLaunchKernelGGL((classify_grad_kernel<KP>), dim3((unsigned)ceil_div(cl->n, CL_BLOCK)), dim3(CL_BLOCK), 0, st, cl->n, S, cl->k,
                           d_x, is_log, (const float *)cl->d_P.p, (const float *)cl->d_dl.p, (const double *)cl->d_loss_s.p,
                           cl->d_G.p, cl->d_lossacc.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

polee_status draw_pass(polee_classify *cl, const float *d_x, int is_log, int32_t S, double scale, bool first, int mode)
{
    switch (cl->KP) {
    case 2: return draw_pass_t<2>(cl, d_x, is_log, S, scale, first, mode);
    case 4: return draw_pass_t<4>(cl, d_x, is_log, S, scale, first, mode);
    case 8: return draw_pass_t<8>(cl, d_x, is_log, S, scale, first, mode);
    default: return draw_pass_t<16>(cl, d_x, is_log, S, scale, first, mode);
    }
}

// mode 0: the Adam step number t; mode 1: gradients to d_gout.  The step's loss goes to d_loss_out[0].
polee_status step_tail(polee_classify *cl, int mode, int64_t t, float *d_loss_out)
{
    polee_ctx *ctx = cl->ctx;
    const polee_classify_opts &o = cl->o;
    const double lr_t = mode == 0 ? (double)o.learning_rate * std::sqrt(1.0 - std::pow((double)o.beta2, (double)t)) /
                                        (1.0 - std::pow((double)o.beta1, (double)t))
                                  : 0.0;
    hipLaunchKernelGGL(classify_update_kernel, dim3((unsigned)ceil_div(cl->total, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, cl->total,
                       cl->kn, cl->d_P.p, cl->d_G.p, cl->d_M.p, cl->d_V.p, (float)lr_t, o.beta1, o.beta2, o.epsilon, o.l1_penalty, mode,
                       cl->d_gout.p, cl->d_lossacc.p, d_loss_out);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// the flat device layout <-> the ABI's w [n][k], x_bias [n], z_bias [k]
void to_abi(const polee_classify *cl, const std::vector<float> &flat, float *w, float *xb, float *zb)
{
    const int64_t n = cl->n, k = cl->k;
    if (w)
        for (int64_t j = 0; j < n; ++j)
            for (int64_t c = 0; c < k; ++c) w[j * k + c] = flat[(size_t)(c * n + j)];
    if (xb) std::copy(flat.begin() + cl->kn, flat.begin() + cl->kn + n, xb);
    if (zb) std::copy(flat.begin() + cl->kn + n, flat.end(), zb);
}

polee_status eval_tail(polee_classify *cl, float *loss, float *g_w, float *g_xb, float *g_zb)
{
    polee_ctx *ctx = cl->ctx;
    POLEE_TRY(step_tail(cl, 1, 0, cl->d_loss.p));
    POLEE_TRY(cl->d_loss.download(ctx, loss, 1));
    if (!g_w && !g_xb && !g_zb) return POLEE_OK;  // (the loss alone: nothing else crosses to the host)
    std::vector<float> flat((size_t)cl->total);
    POLEE_TRY(cl->d_gout.download(ctx, flat.data(), flat.size()));
    to_abi(cl, flat, g_w, g_xb, g_zb);
    return POLEE_OK;
}

// A call that failed between two updates leaves the gradient accumulators and the loss term partly summed: they go back to zero
// (best effort: the status the caller sees is the first failure's), and the clock advances by the steps that did complete, whose
// updates the parameters already hold -- so the next call on the handle neither adds stale sums nor reuses a step number.
polee_status abandon(polee_classify *cl, int64_t steps_done, polee_status st)
{
    polee_ctx *ctx = cl->ctx;
    const std::string msg = ctx->err;
    cl->t += steps_done;
    (void)hipGetLastError();
    (void)hipMemsetAsync(cl->d_G.p, 0, (size_t)cl->total * sizeof(float), ctx->stream);
    (void)hipMemsetAsync(cl->d_lossacc.p, 0, sizeof(double), ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    ctx->err = msg;
    global_error() = msg;
    return st;
}

polee_status fit_finish(polee_classify *cl, int32_t niter, float *loss_trace)
{
    polee_ctx *ctx = cl->ctx;
    cl->t += niter;
    if (loss_trace) return cl->d_loss.download(ctx, loss_trace, (size_t)niter);
    POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return POLEE_OK;
}

polee_status predict_finish(polee_classify *cl, int32_t S, int32_t ndraws, float *probs)
{
    polee_ctx *ctx = cl->ctx;
    const int64_t sk = (int64_t)S * cl->k;
    hipLaunchKernelGGL(classify_probs_kernel, dim3((unsigned)ceil_div(sk, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, sk,
                       (const double *)cl->d_probs.p, (double)ndraws, cl->d_probs_out.p);
    POLEE_KERNEL_CHECK(ctx);
    return cl->d_probs_out.download(ctx, probs, (size_t)sk);
}

}  // namespace

extern "C" {

void polee_classify_default_opts(polee_classify_opts *o)
{
    if (!o) return;
    o->draws_per_step = 5;     // samples_per_iter (polee_classify.py:51)
    o->learning_rate = 1e-4f;  // (:69, :92)
    o->l1_penalty = 1e-3f;     // (:29)
    o->loss_scale = 1.0f;      // (:22)
    o->beta1 = 0.9f;           // tf.optimizers.Adam's defaults
    o->beta2 = 0.999f;
    o->epsilon = 1e-7f;
}

polee_status polee_classify_create(polee_ctx *ctx, int32_t n, int32_t k, const polee_classify_opts *opts, polee_classify **out)
{
    if (!ctx) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_create: null context");
    return guarded(ctx, "polee_classify_create", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        if (!out || n < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_create: bad argument");
        if (k < 2 || k > 16)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_classify_create: %d classes; the kernels are built for 2..16", k);
        polee_classify_opts o;
        polee_classify_default_opts(&o);
        if (opts) o = *opts;
        POLEE_TRY(check_opts(ctx, o));
        polee_classify *cl = new polee_classify();
        cl->ctx = ctx;
        ctx_retain(ctx);
        cl->n = n;
        cl->k = k;
        cl->KP = k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
        cl->nchunks = (int32_t)ceil_div(n, CL_WAVE_J);
        cl->kn = (int64_t)k * n;
        cl->total = cl->kn + n + k;
        cl->o = o;
        polee_status st = POLEE_OK;
        auto A = [&](polee_status s) {
            if (st == POLEE_OK) st = s;
        };
        const size_t tot = (size_t)cl->total;
        A(cl->d_P.alloc(ctx, tot));
        A(cl->d_M.alloc(ctx, tot));
        A(cl->d_V.alloc(ctx, tot));
        A(cl->d_G.alloc(ctx, tot));
        A(cl->d_gout.alloc(ctx, tot));
        A(cl->d_abs.alloc(ctx, (size_t)cl->nchunks));
        A(cl->d_loss.alloc(ctx, 1));
        A(cl->d_lossacc.alloc(ctx, 2));
        if (st == POLEE_OK) {
            hipError_t e = hipSuccess;
            for (float *p : {cl->d_P.p, cl->d_M.p, cl->d_V.p, cl->d_G.p})
                if (e == hipSuccess) e = hipMemsetAsync(p, 0, tot * sizeof(float), ctx->stream);
            if (e == hipSuccess) e = hipMemsetAsync(cl->d_lossacc.p, 0, 2 * sizeof(double), ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) st = fail(ctx, POLEE_ERR_HIP, "polee_classify_create: %s", hipGetErrorString(e));
        }
        if (st != POLEE_OK) {
            polee_classify_destroy(cl);
            return st;
        }
        *out = cl;
        return POLEE_OK;
    });
}

void polee_classify_destroy(polee_classify *cl)
{
    if (!cl) return;
    polee_ctx *ctx = cl->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete cl;
    ctx_release(ctx);
}

polee_status polee_classify_set_opts(polee_classify *cl, const polee_classify_opts *opts)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_set_opts: null handle");
    if (!opts) return fail(cl->ctx, POLEE_ERR_BAD_ARG, "polee_classify_set_opts: null argument");
    POLEE_TRY(check_opts(cl->ctx, *opts));
    cl->o = *opts;
    return POLEE_OK;
}

polee_status polee_classify_get_params(polee_classify *cl, float *w, float *x_bias, float *z_bias)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_get_params: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_get_params", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        std::vector<float> flat((size_t)cl->total);
        POLEE_TRY(cl->d_P.download(ctx, flat.data(), flat.size()));
        to_abi(cl, flat, w, x_bias, z_bias);
        return POLEE_OK;
    });
}

polee_status polee_classify_set_params(polee_classify *cl, const float *w, const float *x_bias, const float *z_bias)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_set_params: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_set_params", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        if (!w || !x_bias || !z_bias) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_set_params: null argument");
        const int64_t n = cl->n, k = cl->k;
        std::vector<float> flat((size_t)cl->total);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t c = 0; c < k; ++c) flat[(size_t)(c * n + j)] = w[j * k + c];
        std::copy(x_bias, x_bias + n, flat.begin() + cl->kn);
        std::copy(z_bias, z_bias + k, flat.begin() + cl->kn + n);
        return cl->d_P.upload(ctx, flat);
    });
}

polee_status polee_classify_reset(polee_classify *cl)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_reset: null handle");
    polee_ctx *ctx = cl->ctx;
    POLEE_TRY(use_device(ctx));
    const size_t bytes = (size_t)cl->total * sizeof(float);
    POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_M.p, 0, bytes, ctx->stream));
    POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_V.p, 0, bytes, ctx->stream));
    POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_G.p, 0, bytes, ctx->stream));
    POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_lossacc.p, 0, 2 * sizeof(double), ctx->stream));
    POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    cl->t = 0;
    return POLEE_OK;
}

polee_status polee_classify_init_bias(polee_classify *cl, polee_approx *ap, const float *z0, uint64_t seed)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_init_bias: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_init_bias", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        int32_t S = 0;
        POLEE_TRY(check_approx(cl, ap, &S));
        if (z0) POLEE_TRY(cl->d_z0.upload(ctx, z0, (size_t)S * (cl->n - 1)));
        POLEE_TRY(approx_sample_device(ap, z0 ? cl->d_z0.p : nullptr, seed));
        hipLaunchKernelGGL(classify_colmean_kernel, dim3((unsigned)ceil_div(cl->n, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, cl->n, S,
                           approx_draw_buffer(ap), 0, cl->d_P.p + cl->kn);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    });
}

polee_status polee_classify_init_bias_points(polee_classify *cl, const float *x, int32_t S)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_init_bias_points: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_init_bias_points", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        POLEE_TRY(upload_points(cl, x, S));
        hipLaunchKernelGGL(classify_colmean_kernel, dim3((unsigned)ceil_div(cl->n, CL_BLOCK)), dim3(CL_BLOCK), 0, ctx->stream, cl->n, S,
                           (const float *)cl->d_x.p, 1, cl->d_P.p + cl->kn);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    });
}

polee_status polee_classify_eval(polee_classify *cl, polee_approx *ap, const float *labels, const float *z0, uint64_t seed, float *loss,
                                 float *g_w, float *g_x_bias, float *g_z_bias)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_eval: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_eval", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        int32_t S = 0;
        POLEE_TRY(check_approx(cl, ap, &S));
        if (!labels || !loss) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_eval: null argument");
        const int32_t D = cl->o.draws_per_step;
        const size_t sk = (size_t)S * (cl->n - 1);
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_TRY(upload_labels(cl, labels, S));
        if (z0) POLEE_TRY(cl->d_z0.upload(ctx, z0, (size_t)D * sk));
        polee_status st = POLEE_OK;
        for (int32_t d = 0; d < D && st == POLEE_OK; ++d) {
            st = approx_sample_device(ap, z0 ? cl->d_z0.p + (size_t)d * sk : nullptr, seed + CL_DRAW_STRIDE * (uint64_t)d);
            if (st == POLEE_OK) st = draw_pass(cl, approx_draw_buffer(ap), 0, S, (double)cl->o.loss_scale / D, d == 0, 0);
        }
        if (st == POLEE_OK) st = eval_tail(cl, loss, g_w, g_x_bias, g_z_bias);
        return st == POLEE_OK ? st : abandon(cl, 0, st);
    });
}

polee_status polee_classify_eval_points(polee_classify *cl, const float *x, int32_t S, const float *labels, float *loss, float *g_w,
                                        float *g_x_bias, float *g_z_bias)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_eval_points: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_eval_points", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        if (!labels || !loss) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_eval_points: null argument");
        POLEE_TRY(upload_points(cl, x, S));
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_TRY(upload_labels(cl, labels, S));
        polee_status st = draw_pass(cl, cl->d_x.p, 1, S, (double)cl->o.loss_scale, true, 0);
        if (st == POLEE_OK) st = eval_tail(cl, loss, g_w, g_x_bias, g_z_bias);
        return st == POLEE_OK ? st : abandon(cl, 0, st);
    });
}

polee_status polee_classify_fit(polee_classify *cl, polee_approx *ap, const float *labels, int32_t niter, uint64_t seed, const float *z0,
                                float *loss_trace)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_fit: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_fit", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        int32_t S = 0;
        POLEE_TRY(check_approx(cl, ap, &S));
        if (!labels || niter < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_fit: bad argument");
        const int32_t D = cl->o.draws_per_step;
        const size_t sk = (size_t)S * (cl->n - 1);
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_TRY(upload_labels(cl, labels, S));
        POLEE_TRY(cl->d_loss.alloc(ctx, (size_t)niter));
        if (z0) POLEE_TRY(cl->d_z0.upload(ctx, z0, (size_t)niter * D * sk));  // (once, before the loop)
        const double scale = (double)cl->o.loss_scale / D;
        for (int32_t it = 0; it < niter; ++it) {
            const int64_t t = cl->t + it + 1;
            polee_status st = POLEE_OK;
            for (int32_t d = 0; d < D && st == POLEE_OK; ++d) {
                const uint64_t i = (uint64_t)(t - 1) * (uint64_t)D + (uint64_t)d;
                st = approx_sample_device(ap, z0 ? cl->d_z0.p + ((size_t)it * D + d) * sk : nullptr, seed + CL_DRAW_STRIDE * i);
                if (st == POLEE_OK) st = draw_pass(cl, approx_draw_buffer(ap), 0, S, scale, d == 0, 0);
            }
            if (st == POLEE_OK) st = step_tail(cl, 0, t, cl->d_loss.p + it);
            if (st != POLEE_OK) return abandon(cl, it, st);
        }
        return fit_finish(cl, niter, loss_trace);
    });
}

polee_status polee_classify_fit_points(polee_classify *cl, const float *x, int32_t S, const float *labels, int32_t niter,
                                       float *loss_trace)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_fit_points: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_fit_points", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        if (!labels || niter < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_fit_points: bad argument");
        POLEE_TRY(upload_points(cl, x, S));
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_TRY(upload_labels(cl, labels, S));
        POLEE_TRY(cl->d_loss.alloc(ctx, (size_t)niter));
        for (int32_t it = 0; it < niter; ++it) {
            polee_status st = draw_pass(cl, cl->d_x.p, 1, S, (double)cl->o.loss_scale, true, 0);
            if (st == POLEE_OK) st = step_tail(cl, 0, cl->t + it + 1, cl->d_loss.p + it);
            if (st != POLEE_OK) return abandon(cl, it, st);
        }
        return fit_finish(cl, niter, loss_trace);
    });
}

// (the two prediction entries return a failure as it is, without abandon(): they touch neither the gradient accumulators nor the loss
// term nor the clock, and their own accumulator d_probs is zeroed at the start of every call)
polee_status polee_classify_predict(polee_classify *cl, polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0, float *probs)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_predict: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_predict", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        int32_t S = 0;
        POLEE_TRY(check_approx(cl, ap, &S));
        if (!probs || ndraws < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_predict: bad argument");
        const size_t sk = (size_t)S * (cl->n - 1);
        POLEE_TRY(ensure_samples(cl, S));
        if (z0) POLEE_TRY(cl->d_z0.upload(ctx, z0, (size_t)ndraws * sk));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_probs.p, 0, (size_t)S * cl->k * sizeof(double), ctx->stream));
        for (int32_t i = 0; i < ndraws; ++i) {
            POLEE_TRY(approx_sample_device(ap, z0 ? cl->d_z0.p + (size_t)i * sk : nullptr, seed + CL_DRAW_STRIDE * (uint64_t)i));
            POLEE_TRY(draw_pass(cl, approx_draw_buffer(ap), 0, S, 1.0, false, 1));
        }
        return predict_finish(cl, S, ndraws, probs);
    });
}

polee_status polee_classify_predict_points(polee_classify *cl, const float *x, int32_t S, float *probs)
{
    if (!cl) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_classify_predict_points: null handle");
    polee_ctx *ctx = cl->ctx;
    return guarded(ctx, "polee_classify_predict_points", [&]() -> polee_status {
        POLEE_TRY(use_device(ctx));
        if (!probs) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_predict_points: null argument");
        POLEE_TRY(upload_points(cl, x, S));
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_probs.p, 0, (size_t)S * cl->k * sizeof(double), ctx->stream));
        POLEE_TRY(draw_pass(cl, cl->d_x.p, 1, S, 1.0, false, 1));
        return predict_finish(cl, S, 1, probs);
    });
}

}  // extern "C"

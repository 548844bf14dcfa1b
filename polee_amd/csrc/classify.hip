// `polee model classify` (models/classify.jl, models/polee_classify.py:13-114): multinomial logistic regression on log expression,
// trained on fresh draws from the training samples' fitted approximations at every step, predicting by the mean class probability over
// draws from the testing samples' approximations.  DESIGN.md section 3.10.
//
//   logits[s][c] = sum_j (lx[s][j] - x_bias[j]) w[j][c] + z_bias[c]           lx = log of a draw, or an uploaded point estimate
//   loss         = loss_scale / D  sum_d sum_s CE(labels_s, softmax(logits_s)) + l1 sum |w|
//
// Per draw, on the context's stream, nothing waits for the device:
//   1. approx_sample_device           the draw x [S][n] (approx.hip), clipped at 1e-16 so logf is finite
//   2. classify_logits_kernel         chunk_project with the bias: partials [chunks][S][k]; on a step's first draw also sum |w|
//   3. classify_finish_kernel         one workgroup per sample: the partials summed in f64 in a fixed order, + z_bias, softmax in f64;
//                                     training: dl = (softmax - labels) loss_scale / D and the sample's loss term; prediction:
//                                     probabilities accumulated in f64
//   4. classify_grad_kernel           grad_accumulate with the bias, one thread per transcript:
//                                     g_w[c][j] += sum_s (lx - x_bias[j]) dl[s][c];  g_xb[j] -= sum_c w[j][c] sum_s dl[s][c];
//                                     workgroup 0 adds the draw's g_zb and loss
// After the last draw of a step classify_update_kernel adds l1 sign(w), applies Adam (tf_adam) to w, x_bias and z_bias and leaves the
// accumulators at zero; in evaluation mode it hands the same gradients out instead.
// The projection, the LDS-tiled gradient accumulation, the f64 sums over chunks, Adam and the draw loop are draw_model.hpp's, shared
// with tsne.hip.  There are no float atomics: every sum has a fixed order, so results are bitwise reproducible.
// Parameters, moments and accumulators share one flat layout: wT [k][n] | x_bias [n] | z_bias [k] (the ABI speaks w [n][k]).
#include "draw_model.hpp"

namespace polee {

// part [nchunks][S][k]; abs_part [nchunks] or null: sum |w| of the chunk (the L1 term of the loss, once per step)
template <int KP>
__global__ __launch_bounds__(DM_BLOCK) void classify_logits_kernel(int n, int S, int k, int nchunks, const float *__restrict__ x,
                                                                  int is_log, const float *__restrict__ P,
                                                                  float *__restrict__ part, float *__restrict__ abs_part)
{
    chunk_project<KP, true, false>(n, S, k, nchunks, x, is_log, P, P + (int64_t)k * n, part, abs_part, nullptr);
}

// grid S (+ 1 when abs_part: that workgroup sums the L1 term into lossacc[1]).  mode 0: dl [S][k], loss_s [S]; mode 1: probs [S][k] +=
template <int KP>
__global__ __launch_bounds__(DM_BLOCK) void classify_finish_kernel(int S, int k, int nchunks, const float *__restrict__ part,
                                                                  const float *__restrict__ zb, const float *__restrict__ labels,
                                                                  double scale, int mode, float *__restrict__ dl,
                                                                  double *__restrict__ loss_s, double *__restrict__ probs,
                                                                  const float *__restrict__ abs_part, double l1,
                                                                  double *__restrict__ lossacc)
{
    __shared__ double red[DM_BLOCK];
    const int tid = threadIdx.x, s = blockIdx.x;
    if (s == S) {  // (only launched with abs_part)
        double a = 0.0;
        for (int ch = tid; ch < nchunks; ch += DM_BLOCK) a += (double)abs_part[ch];
        a = block_sum(a, red);
        if (tid == 0) lossacc[1] = l1 * a;
        return;
    }
    chunk_sum<KP, false>(part, S, k, nchunks, s, red);
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
__global__ __launch_bounds__(DM_BLOCK) void classify_grad_kernel(int n, int S, int k, const float *__restrict__ x, int is_log,
                                                                const float *__restrict__ P, const float *__restrict__ dl,
                                                                const double *__restrict__ loss_s, float *__restrict__ G,
                                                                double *__restrict__ lossacc)
{
    __shared__ float sdl[DM_TILE_S * KP];
    __shared__ float sds[KP];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * DM_BLOCK + tid;
    const bool active = j < n;
    const int64_t kn = (int64_t)k * n;
    const float xbj = active ? P[kn + j] : 0.0f;
    float acc[KP];
    double dsum;
    grad_accumulate<KP, true, true>(n, S, k, x, is_log, dl, j, active, xbj, sdl, acc, dsum);
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

// After the last draw of a step.  mode 0: Adam; mode 1: the gradients go to gout, nothing is updated.  Either way the accumulators are
// left at zero and loss_out[0] = the step's loss.
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
    P[i] = tf_adam(p, &M[i], &V[i], g, lr_t, b1, b2, eps);
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

polee_status upload_points(polee_classify *cl, const float *x, int32_t S)
{
    POLEE_TRY(check_points(cl->ctx, "polee_classify", x, S, cl->n));
    return cl->d_x.upload(cl->ctx, x, (size_t)S * cl->n);
}

// one draw through the kernels.  mode 0: training (dl, loss, gradient accumulation), 1: prediction (probabilities accumulated)
template <int KP>
polee_status draw_pass_t(polee_classify *cl, const float *d_x, int is_log, int32_t S, double scale, bool first, int mode)
{
    polee_ctx *ctx = cl->ctx;
    hipStream_t st = ctx->stream;
    const bool pen = first && mode == 0;
    hipLaunchKernelGGL((classify_logits_kernel<KP>), dim3((unsigned)ceil_div(cl->nchunks, DM_BLOCK / 64)), dim3(DM_BLOCK), 0, st, cl->n, S,
                       cl->k, cl->nchunks, d_x, is_log, (const float *)cl->d_P.p, cl->d_part.p, pen ? cl->d_abs.p : nullptr);
    hipLaunchKernelGGL((classify_finish_kernel<KP>), dim3((unsigned)(S + (pen ? 1 : 0))), dim3(DM_BLOCK), 0, st, S, cl->k, cl->nchunks,
                       (const float *)cl->d_part.p, (const float *)(cl->d_P.p + cl->kn + cl->n), (const float *)cl->d_labels.p, scale,
                       mode, cl->d_dl.p, cl->d_loss_s.p, cl->d_probs.p, (const float *)(pen ? cl->d_abs.p : nullptr),
                       (double)cl->o.l1_penalty, cl->d_lossacc.p);
    if (mode == 0)
        hipLaunchKernelGGL((classify_grad_kernel<KP>), dim3((unsigned)ceil_div(cl->n, DM_BLOCK)), dim3(DM_BLOCK), 0, st, cl->n, S, cl->k,
                           d_x, is_log, (const float *)cl->d_P.p, (const float *)cl->d_dl.p, (const double *)cl->d_loss_s.p,
                           cl->d_G.p, cl->d_lossacc.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

polee_status draw_pass(polee_classify *cl, const float *d_x, int is_log, int32_t S, double scale, bool first, int mode)
{
    return dispatch_kp(cl->KP, [&](auto kp) { return draw_pass_t<decltype(kp)::value>(cl, d_x, is_log, S, scale, first, mode); });
}

// mode 0: the Adam step number t; mode 1: gradients to d_gout.  The step's loss goes to d_loss_out[0].
polee_status step_tail(polee_classify *cl, int mode, int64_t t, float *d_loss_out)
{
    polee_ctx *ctx = cl->ctx;
    const polee_classify_opts &o = cl->o;
    const double lr_t = mode == 0 ? tf_adam_rate(o.learning_rate, o.beta1, o.beta2, t) : 0.0;
    hipLaunchKernelGGL(classify_update_kernel, dim3((unsigned)ceil_div(cl->total, DM_BLOCK)), dim3(DM_BLOCK), 0, ctx->stream, cl->total,
                       cl->kn, cl->d_P.p, cl->d_G.p, cl->d_M.p, cl->d_V.p, (float)lr_t, o.beta1, o.beta2, o.epsilon, o.l1_penalty, mode,
                       cl->d_gout.p, cl->d_lossacc.p, d_loss_out);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// the flat device layout <-> the ABI's w [n][k], x_bias [n], z_bias [k]
void to_abi(const polee_classify *cl, const std::vector<float> &flat, float *w, float *xb, float *zb)
{
    if (w) wT_to_abi(flat.data(), cl->n, cl->k, w);
    if (xb) std::copy(flat.begin() + cl->kn, flat.begin() + cl->kn + cl->n, xb);
    if (zb) std::copy(flat.begin() + cl->kn + cl->n, flat.end(), zb);
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

polee_status predict_finish(polee_classify *cl, int32_t S, int32_t ndraws, float *probs)
{
    polee_ctx *ctx = cl->ctx;
    const int64_t sk = (int64_t)S * cl->k;
    POLEE_TRY(launch_acc_mean(ctx, sk, cl->d_probs.p, ndraws, cl->d_probs_out.p));
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
    return ctx_entry(ctx, "polee_classify_create", [&]() -> polee_status {
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
        cl->KP = kp_of(k);
        cl->nchunks = (int32_t)ceil_div(n, DM_WAVE_J);
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
    return entry(cl, "polee_classify_set_opts", [&](polee_ctx *ctx) -> polee_status {
        if (!opts) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_set_opts: null argument");
        POLEE_TRY(check_opts(ctx, *opts));
        cl->o = *opts;
        return POLEE_OK;
    });
}

polee_status polee_classify_get_params(polee_classify *cl, float *w, float *x_bias, float *z_bias)
{
    return entry(cl, "polee_classify_get_params", [&](polee_ctx *ctx) -> polee_status {
        std::vector<float> flat((size_t)cl->total);
        POLEE_TRY(cl->d_P.download(ctx, flat.data(), flat.size()));
        to_abi(cl, flat, w, x_bias, z_bias);
        return POLEE_OK;
    });
}

polee_status polee_classify_set_params(polee_classify *cl, const float *w, const float *x_bias, const float *z_bias)
{
    return entry(cl, "polee_classify_set_params", [&](polee_ctx *ctx) -> polee_status {
        if (!w || !x_bias || !z_bias) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_set_params: null argument");
        std::vector<float> flat((size_t)cl->total);
        abi_to_wT(w, cl->n, cl->k, flat.data());
        std::copy(x_bias, x_bias + cl->n, flat.begin() + cl->kn);
        std::copy(z_bias, z_bias + cl->k, flat.begin() + cl->kn + cl->n);
        return cl->d_P.upload(ctx, flat);
    });
}

polee_status polee_classify_reset(polee_classify *cl)
{
    return entry(cl, "polee_classify_reset", [&](polee_ctx *ctx) -> polee_status {
        const size_t bytes = (size_t)cl->total * sizeof(float);
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_M.p, 0, bytes, ctx->stream));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_V.p, 0, bytes, ctx->stream));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_G.p, 0, bytes, ctx->stream));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_lossacc.p, 0, 2 * sizeof(double), ctx->stream));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        cl->t = 0;
        return POLEE_OK;
    });
}

polee_status polee_classify_init_bias(polee_classify *cl, polee_approx *ap, const float *z0, uint64_t seed)
{
    return entry(cl, "polee_classify_init_bias", [&](polee_ctx *ctx) -> polee_status {
        int32_t S = 0;
        POLEE_TRY(check_approx(ctx, "polee_classify", ap, cl->n, 0, &S));
        DrawFeed feed(ap, cl->d_z0, S, cl->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, 1));
        POLEE_TRY(feed.draw(0, 0, &d_x));
        hipLaunchKernelGGL(classify_colmean_kernel, dim3((unsigned)ceil_div(cl->n, DM_BLOCK)), dim3(DM_BLOCK), 0, ctx->stream, cl->n, S,
                           d_x, 0, cl->d_P.p + cl->kn);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    });
}

polee_status polee_classify_init_bias_points(polee_classify *cl, const float *x, int32_t S)
{
    return entry(cl, "polee_classify_init_bias_points", [&](polee_ctx *ctx) -> polee_status {
        POLEE_TRY(upload_points(cl, x, S));
        hipLaunchKernelGGL(classify_colmean_kernel, dim3((unsigned)ceil_div(cl->n, DM_BLOCK)), dim3(DM_BLOCK), 0, ctx->stream, cl->n, S,
                           (const float *)cl->d_x.p, 1, cl->d_P.p + cl->kn);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    });
}

polee_status polee_classify_eval(polee_classify *cl, polee_approx *ap, const float *labels, const float *z0, uint64_t seed, float *loss,
                                 float *g_w, float *g_x_bias, float *g_z_bias)
{
    return entry(cl, "polee_classify_eval", [&](polee_ctx *ctx) -> polee_status {
        int32_t S = 0;
        POLEE_TRY(check_approx(ctx, "polee_classify", ap, cl->n, 0, &S));
        if (!labels || !loss) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_eval: null argument");
        const int32_t D = cl->o.draws_per_step;
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_TRY(upload_labels(cl, labels, S));
        DrawFeed feed(ap, cl->d_z0, S, cl->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)D));
        polee_status st = POLEE_OK;
        for (int32_t d = 0; d < D && st == POLEE_OK; ++d) {
            st = feed.draw((uint64_t)d, (size_t)d, &d_x);
            if (st == POLEE_OK) st = draw_pass(cl, d_x, 0, S, (double)cl->o.loss_scale / D, d == 0, 0);
        }
        if (st == POLEE_OK) st = eval_tail(cl, loss, g_w, g_x_bias, g_z_bias);
        return st == POLEE_OK ? st : abandon(cl, 0, st);
    });
}

polee_status polee_classify_eval_points(polee_classify *cl, const float *x, int32_t S, const float *labels, float *loss, float *g_w,
                                        float *g_x_bias, float *g_z_bias)
{
    return entry(cl, "polee_classify_eval_points", [&](polee_ctx *ctx) -> polee_status {
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
    return entry(cl, "polee_classify_fit", [&](polee_ctx *ctx) -> polee_status {
        int32_t S = 0;
        POLEE_TRY(check_approx(ctx, "polee_classify", ap, cl->n, 0, &S));
        if (!labels || niter < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_fit: bad argument");
        const int32_t D = cl->o.draws_per_step;
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_TRY(upload_labels(cl, labels, S));
        POLEE_TRY(cl->d_loss.alloc(ctx, (size_t)niter));
        DrawFeed feed(ap, cl->d_z0, S, cl->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)niter * D));
        const double scale = (double)cl->o.loss_scale / D;
        for (int32_t it = 0; it < niter; ++it) {
            const int64_t t = cl->t + it + 1;
            polee_status st = POLEE_OK;
            for (int32_t d = 0; d < D && st == POLEE_OK; ++d) {
                st = feed.draw((uint64_t)(t - 1) * (uint64_t)D + (uint64_t)d, (size_t)it * D + d, &d_x);
                if (st == POLEE_OK) st = draw_pass(cl, d_x, 0, S, scale, d == 0, 0);
            }
            if (st == POLEE_OK) st = step_tail(cl, 0, t, cl->d_loss.p + it);
            if (st != POLEE_OK) return abandon(cl, it, st);
        }
        return fit_finish(ctx, &cl->t, cl->d_loss, niter, loss_trace);
    });
}

polee_status polee_classify_fit_points(polee_classify *cl, const float *x, int32_t S, const float *labels, int32_t niter,
                                       float *loss_trace)
{
    return entry(cl, "polee_classify_fit_points", [&](polee_ctx *ctx) -> polee_status {
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
        return fit_finish(ctx, &cl->t, cl->d_loss, niter, loss_trace);
    });
}

// (the two prediction entries return a failure as it is, without abandon(): they touch neither the gradient accumulators nor the loss
// term nor the clock, and their own accumulator d_probs is zeroed at the start of every call)
polee_status polee_classify_predict(polee_classify *cl, polee_approx *ap, int32_t ndraws, uint64_t seed, const float *z0, float *probs)
{
    return entry(cl, "polee_classify_predict", [&](polee_ctx *ctx) -> polee_status {
        int32_t S = 0;
        POLEE_TRY(check_approx(ctx, "polee_classify", ap, cl->n, 0, &S));
        if (!probs || ndraws < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_predict: bad argument");
        POLEE_TRY(ensure_samples(cl, S));
        DrawFeed feed(ap, cl->d_z0, S, cl->n, seed);
        const float *d_x = nullptr;
        POLEE_TRY(feed.upload(z0, (size_t)ndraws));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_probs.p, 0, (size_t)S * cl->k * sizeof(double), ctx->stream));
        for (int32_t i = 0; i < ndraws; ++i) {
            POLEE_TRY(feed.draw((uint64_t)i, (size_t)i, &d_x));
            POLEE_TRY(draw_pass(cl, d_x, 0, S, 1.0, false, 1));
        }
        return predict_finish(cl, S, ndraws, probs);
    });
}

polee_status polee_classify_predict_points(polee_classify *cl, const float *x, int32_t S, float *probs)
{
    return entry(cl, "polee_classify_predict_points", [&](polee_ctx *ctx) -> polee_status {
        if (!probs) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_classify_predict_points: null argument");
        POLEE_TRY(upload_points(cl, x, S));
        POLEE_TRY(ensure_samples(cl, S));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(cl->d_probs.p, 0, (size_t)S * cl->k * sizeof(double), ctx->stream));
        POLEE_TRY(draw_pass(cl, cl->d_x.p, 1, S, 1.0, false, 1));
        return predict_finish(cl, S, 1, probs);
    });
}

}  // extern "C"

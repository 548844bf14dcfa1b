// The alternative likelihood approximations' VI loop, device resident.
// Replaces approximate_likelihood(::LogisticNormalApprox, sample) (src/likelihood-approximation-alt.jl:50-203),
// (::NormalILRApprox, sample) (:503-616 with src/isometric_log_ratios.jl:43-128) and (::NormalALRApprox, sample)
// (:619-736 with src/additive_log_ratios.jl:12-71), ADAM (src/likelihood-approximation.jl:107-146), and their samplers
// (sample_likap, src/evaluate.jl:34-74, 203-275).  The two Polya-tree alternatives (logit_normal_ptt, kumaraswamy_ptt)
// are named in the method enum and not built: polee_altvi_create answers them with POLEE_ERR_UNSUPPORTED.
//
// All three methods end in a softmax over n log-values eta (one of them fixed at 0 for the two that have a reference
// element), so one set of kernels serves them.  One VI iteration, the K draws side by side:
//   [ILR] tour scan     : eta = prefix of a*y / b*y over the Euler tour (scan.hpp, 3 launches)   -> eta [K][n] f64, leaf order
//   stats + finish      : per block (max, sum exp(eta - max)); fixed-order second stage            -> M, S [K]
//   apply               : x = clamp(exp(eta - M) / S), g = 0, per-block side sums                  -> x, g [n][K] f32
//   loglik              : loglik_eval_device, one sparse pass for all K draws                      -> g, lp
//   dot + finish        : c = sum x (g [+ 1/x]) per block in f64; fixed-order second stage         -> c, xsum, ladj [K]
//   [ILR] leaf scan     : prefix over leaf order of the leaf gradients in f64 (3 launches)         -> P [K][n+1]
//   update              : y_grad per parameter, mean over K, ADAM on mu and omega, the next step's noise
// The softmax subtracts the maximum: it equals the reference's exp / sum / divide wherever the reference's Float32 exp
// neither overflows nor underflows.  No float atomics and no host synchronisation inside polee_altvi_run; the number of
// launches does not depend on the tree.
#include "adam.hpp"
#include "loglik_internal.hpp"
#include "ptt_internal.hpp"
#include "rng.hpp"

#include <cmath>

namespace polee {

constexpr int ALT_THREADS = 256;
constexpr int ALT_MAX_BLOCKS = 256;

// where a draw's log-values come from
struct AltEta {
    const double *eta;        // ILR: [K][n] by leaf position; null for the two softmax methods
    const int32_t *leaf_tid;  // ILR: leaf position -> transcript
    const float *mu, *omega, *z;  // z [K][n-1]
    int32_t n, ref;           // ref: the 0-based element whose log-value is 0 (logistic-normal: n - 1; ALR: refidx - 1; ILR: -1)
    __device__ inline float y(int d, int64_t j) const
    {
        // ys[i] = mu[i] + sigma[i] * zs[i] in Float32, sigma = exp(omega) (likelihood-approximation-alt.jl:106,120,571,690)
        return mu[j] + expf(omega[j]) * z[(int64_t)d * (n - 1) + j];
    }
    __device__ inline double get(int d, int64_t i) const
    {
        if (eta) return eta[(int64_t)d * n + i];
        if (i == ref) return 0.0;
        return (double)y(d, i < ref ? i : i - 1);
    }
    __device__ inline int64_t tid(int64_t i) const { return leaf_tid ? (int64_t)leaf_tid[i] : i; }
};

__device__ inline double alt_block_max(double v, double *smem4)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) smem4[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = fmax(fmax(smem4[0], smem4[1]), fmax(smem4[2], smem4[3]));
    __syncthreads();
    return r;
}

// per block and draw: the maximum of its elements and the sum of exp(eta - that maximum)
__global__ __launch_bounds__(ALT_THREADS) void alt_softmax_stats_kernel(AltEta e, double *part /* [K][nblk][2] */)
{
    __shared__ double sm[4];
    const int d = blockIdx.y;
    const int64_t stride = (int64_t)gridDim.x * ALT_THREADS;
    double mx = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * ALT_THREADS + threadIdx.x; i < e.n; i += stride) mx = fmax(mx, e.get(d, i));
    mx = alt_block_max(mx, sm);
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * ALT_THREADS + threadIdx.x; i < e.n; i += stride) s += exp(e.get(d, i) - mx);
    s = block_sum_f64(s, sm);
    if (threadIdx.x == 0) {
        part[((int64_t)d * gridDim.x + blockIdx.x) * 2 + 0] = mx;
        part[((int64_t)d * gridDim.x + blockIdx.x) * 2 + 1] = s;
    }
}

// a wave's sum / maximum by a fixed xor tree: every lane gets the result, the same bits on every run
__device__ inline double alt_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline double alt_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// the fixed second stage, one wave per draw (64 * K threads): M = max over blocks, S = sum over blocks; a lane takes every 64th
// block in order, the lanes' partials meet in the xor tree
__global__ void alt_softmax_finish_kernel(const double *part, int nblk, int K, double *ms /* [K][2] */)
{
    const int d = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double M = -INFINITY;
    for (int b = lane; b < nblk; b += 64) M = fmax(M, part[((int64_t)d * nblk + b) * 2]);
    M = alt_wave_max(M);
    double S = 0.0;
    for (int b = lane; b < nblk; b += 64) S += part[((int64_t)d * nblk + b) * 2 + 1] * exp(part[((int64_t)d * nblk + b) * 2] - M);
    S = alt_wave_sum(S);
    if (lane == 0) {
        ms[d * 2 + 0] = M;
        ms[d * 2 + 1] = S;
    }
}

// xs = clamp(exp(eta) / sum, eps, 1 - eps) as Float32 (likelihood-approximation-alt.jl:124-133, 574-575, 693-694); g = 0 for
// the sparse pass; per-block side sums over the elements other than the reference one: xs, log xs, eta
__global__ __launch_bounds__(ALT_THREADS) void alt_softmax_apply_kernel(AltEta e, const double *ms, int K, float lo, float hi, float *x,
                                                                        float *g, double *part /* [K][nblk][3] */)
{
    __shared__ double sm[4];
    const int d = blockIdx.y;
    const int64_t stride = (int64_t)gridDim.x * ALT_THREADS;
    const double M = ms[d * 2], S = ms[d * 2 + 1];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * ALT_THREADS + threadIdx.x; i < e.n; i += stride) {
        const double et = e.get(d, i);
        const float xu = (float)(exp(et - M) / S);
        const float xf = fminf(fmaxf(xu, lo), hi);
        const int64_t t = e.tid(i);
        x[t * K + d] = xf;
        if (g) g[t * K + d] = 0.0f;
        if (i != e.ref) {
            s0 += (double)xf;
            // (ilr_transform! sums log x inside the transform, before the fit clamps xs, isometric_log_ratios.jl:77-83; the
            // logistic-normal's ln_ladj is taken from the clamped xs, likelihood-approximation-alt.jl:133, 157-160)
            s1 += log((double)(e.eta ? xu : xf));
            s2 += et;
        }
    }
    s0 = block_sum_f64(s0, sm);
    s1 = block_sum_f64(s1, sm);
    s2 = block_sum_f64(s2, sm);
    if (threadIdx.x == 0 && part) {
        double *p = part + ((int64_t)d * gridDim.x + blockIdx.x) * 3;
        p[0] = s0;
        p[1] = s1;
        p[2] = s2;
    }
}

// c = sum xs[i] * x_grad[i] (likelihood-approximation-alt.jl:138-141, additive_log_ratios.jl:55-58); ILR adds
// dladj_dxi = 1 / xs[i] to every x_grad[i] (isometric_log_ratios.jl:96-100, with the division by xs_sum taken out)
__global__ __launch_bounds__(ALT_THREADS) void alt_dot_kernel(const float *x, const float *g, int K, int64_t n, int ilr, double *part /* [K][nblk] */)
{
    __shared__ double sm[4];
    const int d = blockIdx.y;
    const int64_t stride = (int64_t)gridDim.x * ALT_THREADS;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * ALT_THREADS + threadIdx.x; i < n; i += stride) {
        const double xs = (double)x[i * K + d];
        s += xs * ((double)g[i * K + d] + (ilr ? 1.0 / xs : 0.0));
    }
    s = block_sum_f64(s, sm);
    if (threadIdx.x == 0) part[(int64_t)d * gridDim.x + blockIdx.x] = s;
}

// per draw: c, xsum and the method's ladj, from the block partials in a fixed order
//   logistic-normal: ln_ladj = log(1 + xsum) + sum log xs[1:n-1], xsum taken after normalisation (:148-160)
//   ALR: sum(ys) - log(1 + sum(exp.(ys))) (additive_log_ratios.jl:27)
//   ILR: sum log xs + log(sqrt(n)) (isometric_log_ratios.jl:77-83)
__global__ void alt_draw_finish_kernel(int method, const double *part_apply, const double *part_dot, const double *ms, int nblk, int K,
                                       int64_t n, double *st /* [K][4]: c, xsum, ladj */)
{
    const int d = threadIdx.x >> 6, lane = threadIdx.x & 63;  // one wave per draw, as alt_softmax_finish_kernel
    double c = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int b = lane; b < nblk; b += 64) {
        if (part_dot) c += part_dot[(int64_t)d * nblk + b];
        const double *p = part_apply + ((int64_t)d * nblk + b) * 3;
        s0 += p[0];
        s1 += p[1];
        s2 += p[2];
    }
    c = alt_wave_sum(c);
    s0 = alt_wave_sum(s0);
    s1 = alt_wave_sum(s1);
    s2 = alt_wave_sum(s2);
    if (lane != 0) return;
    double ladj;
    if (method == POLEE_ALT_LOGISTIC_NORMAL) ladj = log(1.0 + s0) + s1;
    else if (method == POLEE_ALT_NORMAL_ALR) ladj = s2 - (ms[d * 2] + log(ms[d * 2 + 1]));
    else ladj = s1 + log(sqrt((double)n));
    st[d * 4 + 0] = c;
    st[d * 4 + 1] = s0;
    st[d * 4 + 2] = ladj;
}

// ---- ILR over the tree ---------------------------------------------------------------------------------------------------
// ilr_transform! (isometric_log_ratios.jl:43-72): a child's log-value is its parent's plus a * y_k (left) or b * y_k (right):
// the prefix over the Euler tour of +value at a node's ENTER and -value at its EXIT, as the Polya tree's forward scan.
struct AltTourLoad {
    PttView v;
    AltEta e;
    const double *ab;  // [n-1][2]: a, b of every internal node
    __device__ inline double edge(uint32_t code, int row) const
    {
        if (code & 4u) return 0.0;  // the root has no incoming edge
        const int64_t k = code >> 4;
        return ab[2 * k + ((code & 8u) ? 0 : 1)] * (double)e.y(row, k);
    }
    __device__ double operator()(int row, int64_t idx) const
    {
        const uint32_t code = v.tour_code[idx];
        const uint32_t type = code & 3u;
        if (type == TOUR_LEAF) return 0.0;
        const double val = edge(code, row);
        return type == TOUR_ENTER ? val : -val;
    }
};
struct AltTourEmit {
    AltTourLoad ld;
    double *eta;  // [K][n] by leaf position
    __device__ void operator()(int row, int64_t idx, double /*excl*/, double incl) const
    {
        const uint32_t code = ld.v.tour_code[idx];
        if ((code & 3u) == TOUR_LEAF) eta[(int64_t)row * ld.v.n + ld.v.tour_tgt[idx]] = incl + ld.edge(code, row);
    }
};
// ilr_transform_gradients! (isometric_log_ratios.jl:104-110): a leaf's gradient is
//   exp(input_value) * ((1 / xs_sum) * (x_grad + 1 / xs) - c)  =  (exp(eta) / xs_sum) * (x_grad + 1 / xs - c'),  c' = xs_sum * c,
// with exp(eta) / xs_sum the normalised value before the clamp, and xs the clamped one; an internal node's gradient is the
// sum over its leaves (:121): the prefix P over leaf order, in f64
struct AltLeafGradLoad {
    AltEta e;
    const double *ms, *st;
    const float *x, *g;
    int K;
    __device__ double operator()(int row, int64_t pos) const
    {
        const int64_t t = e.tid(pos);
        const double xs = (double)x[t * K + row];
        const double xt = exp(e.get(row, pos) - ms[row * 2]) / ms[row * 2 + 1];
        return xt * ((double)g[t * K + row] + 1.0 / xs - st[row * 4]);
    }
};
struct AltPrefixEmit {
    int64_t n;
    double *P;  // [K][n+1]
    __device__ void operator()(int row, int64_t pos, double excl, double incl) const
    {
        P[(int64_t)row * (n + 1) + pos] = excl;
        if (pos == n - 1) P[(int64_t)row * (n + 1) + n] = incl;
    }
};

// ---- update ----------------------------------------------------------------------------------------------------------------
// adam_update_mv! and adam_update_params! (likelihood-approximation.jl:116-146)
__device__ inline void alt_adam_one(float &p, float &m, float &v, float grad, const AdamConsts &a, double max_step)
{
    if (a.first) {
        m = grad;
        v = grad * grad;
    } else {
        m = (float)(a.rm * (double)m + (1 - a.rm) * (double)grad);
        v = (float)(a.rv * (double)v + (1 - a.rv) * (double)(grad * grad));
    }
    const double pm = (double)m * a.inv_m_denom, pv = (double)v * a.inv_v_denom;
    double delta = a.lr * pm / (sqrt(pv) + a.eps);
    delta = delta < -max_step ? -max_step : (delta > max_step ? max_step : delta);
    p = (float)((double)p + delta);
}

struct AltUpd {
    int method, K, apply, step;
    int64_t n;
    AltEta e;
    const float *x, *g;
    const double *st, *P, *ab;
    const int32_t *lo, *mid, *hi1;
    float *mu, *omega, *m0, *v0, *m1, *v1;
    AdamConsts adam;  // (max_mu, max_omega: the caps of the two parameter vectors)
    int *flag;
    double *ygrad;        // hook: [K][n-1] or null
    float *mug, *omg;     // hook: [n-1] or null
    float *znext;         // [K][n-1] the next step's noise, or null
    uint64_t seed;
};
__global__ __launch_bounds__(ALT_THREADS) void alt_update_kernel(AltUpd u)
{
    const int64_t j = (int64_t)blockIdx.x * ALT_THREADS + threadIdx.x;
    const int64_t nm1 = u.n - 1;
    if (j >= nm1) return;
    const float sigma = expf(u.omega[j]);
    float mug = 0.0f, omg = 0.0f;
    for (int d = 0; d < u.K; ++d) {
        double yg;
        if (u.method == POLEE_ALT_NORMAL_ILR) {
            // y_grad[k] = a * left_grad + b * right_grad (isometric_log_ratios.jl:122); left leaves [mid, hi1), right [lo, mid)
            const double *P = u.P + (int64_t)d * (u.n + 1);
            const double pl = P[u.lo[j]], pm = P[u.mid[j]], ph = P[u.hi1[j]];
            yg = u.ab[2 * j] * (ph - pm) + u.ab[2 * j + 1] * (pm - pl);
        } else {
            const int64_t i = j < u.e.ref ? j : j + 1;
            const double xs = (double)u.x[i * u.K + d], gg = (double)u.g[i * u.K + d];
            const double c = u.st[d * 4], xsum = u.st[d * 4 + 1];
            yg = xs * gg - xs * c;
            if (u.method == POLEE_ALT_LOGISTIC_NORMAL)  // (:154, as written)
                yg += (1.0 / (1.0 + xsum)) * (xs - xs * xsum) + 1.0 - xs * (double)(u.n - 1);
            else  // (additive_log_ratios.jl:69, as written)
                yg += 1.0 - xs;
        }
        const float yg32 = (float)yg;  // y_grad is Float32
        if (u.ygrad) u.ygrad[(int64_t)d * nm1 + j] = yg;
        mug += yg32;
        omg += sigma * (u.e.z[(int64_t)d * nm1 + j] * yg32);  // sigma_grad = zs * y_grad; omega_grad += sigma * sigma_grad
    }
    mug /= (float)u.K;
    omg /= (float)u.K;
    if (u.mug) u.mug[j] = mug;
    if (u.omg) u.omg[j] = omg;
    if (!(isfinite(mug) && isfinite(omg))) {
        atomicCAS(u.flag, 0, u.step);
    } else if (u.apply) {
        float p = u.mu[j], m = u.m0[j], v = u.v0[j];
        alt_adam_one(p, m, v, mug, u.adam, u.adam.max_mu);
        u.mu[j] = p;
        u.m0[j] = m;
        u.v0[j] = v;
        p = u.omega[j], m = u.m1[j], v = u.v1[j];
        alt_adam_one(p, m, v, omg, u.adam, u.adam.max_omega);
        u.omega[j] = p;
        u.m1[j] = m;
        u.v1[j] = v;
    }
    if (u.znext)
        for (int d = 0; d < u.K; ++d) u.znext[(int64_t)d * nm1 + j] = philox_randn(u.seed, (uint32_t)(u.step + 1), (uint32_t)d, (uint32_t)j);
}

__global__ void alt_noise_kernel(uint64_t seed, int step, int64_t nm1, float *z)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int d = blockIdx.y;
    if (k < nm1) z[(int64_t)d * nm1 + k] = philox_randn(seed, (uint32_t)step, (uint32_t)d, (uint32_t)k);
}

// logistic-normal: `elbo = lp + ln_ladj` is an assignment inside the draw loop, then `/= K` (:162, 180): the last draw's
// value over K.  ILR and ALR accumulate (`elbo +=`, :579, 698).
__global__ void alt_trace_kernel(int method, const double *lp, const double *st, int K, int idx, double *elbo, double *lp_mean)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, e = 0.0;
    for (int d = 0; d < K; ++d) {
        s += lp[d];
        e += lp[d] + st[d * 4 + 2];
    }
    if (method == POLEE_ALT_LOGISTIC_NORMAL) e = lp[K - 1] + st[(K - 1) * 4 + 2];
    elbo[idx] = e / K;
    lp_mean[idx] = s / K;
}

__global__ void alt_rows_kernel(const float *in, int K, int64_t n, float *out32, double *out64)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int d = (int)(i / n);
    const int64_t j = i - (int64_t)d * n;
    if (out32) out32[i] = in[j * K + d];
    if (out64) out64[i] = (double)in[j * K + d];
}

// sample_likap (evaluate.jl:65-68, 229-232, 266-269): xs[j] /= effective_lengths[j]; xs ./= sum(xs)
__global__ __launch_bounds__(ALT_THREADS) void alt_sample_sum_kernel(const float *x, const float *efflens, int K, int64_t n, double *part)
{
    __shared__ double sm[4];
    const int d = blockIdx.y;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * ALT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ALT_THREADS)
        s += (double)(x[i * K + d] / efflens[i]);
    s = block_sum_f64(s, sm);
    if (threadIdx.x == 0) part[(int64_t)d * gridDim.x + blockIdx.x] = s;
}
__global__ void alt_sample_write_kernel(const float *x, const float *efflens, const double *part, int nblk, int K, int64_t n, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int d = blockIdx.y;
    if (i >= n) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(int64_t)d * nblk + b];
    out[(int64_t)d * n + i] = (x[i * K + d] / efflens[i]) / (float)s;
}

// What the forward pass needs: shared by the fit and the sampler.
struct AltCore {
    polee_ctx *ctx = nullptr;
    polee_ptt *t = nullptr;  // ILR only
    int method = 0;
    int32_t n = 0, K = 0, ref = -1, nblk = 1;
    double eps = 1e-10;
    bool tree_retained = false;
    DevBuf<float> d_mu, d_omega, d_z, d_x;
    DevBuf<double> d_eta, d_ab, d_chunk, d_part_stats, d_part_apply, d_ms;

    polee_status init(polee_ctx *c, int m, polee_ptt *tree, int32_t n_, int32_t K_, int32_t refidx)
    {
        ctx = c;
        method = m;
        t = tree;
        n = n_;
        K = K_;
        if (n < 2) return fail(ctx, POLEE_ERR_BAD_ARG, "the alternative approximations need at least two transcripts");
        if (K < 1 || K > PSELL_MAX_K) return fail(ctx, POLEE_ERR_BAD_ARG, "num_mc_samples must be in 1..8");
        if (method == POLEE_ALT_LOGIT_NORMAL_PTT || method == POLEE_ALT_KUMARASWAMY_PTT)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "approximation method %d (logit_normal_ptt, kumaraswamy_ptt) is not built", method);
        if (method != POLEE_ALT_LOGISTIC_NORMAL && method != POLEE_ALT_NORMAL_ILR && method != POLEE_ALT_NORMAL_ALR)
            return fail(ctx, POLEE_ERR_BAD_ARG, "unknown approximation method %d", method);
        if (method == POLEE_ALT_NORMAL_ILR) {
            if (!t) return fail(ctx, POLEE_ERR_BAD_ARG, "normal_ilr needs a tree");
            if (t->ctx != ctx) return fail(ctx, POLEE_ERR_BAD_ARG, "tree belongs to a different context");
            if (t->T != 1 || t->n != n) return fail(ctx, POLEE_ERR_BAD_ARG, "normal_ilr needs a single tree with %d leaves (got %d)", n, t->n);
            ref = -1;
        } else if (method == POLEE_ALT_NORMAL_ALR) {
            // refidx = reference_idx == -1 ? n : reference_idx (likelihood-approximation-alt.jl:641); 1-based
            if (refidx == -1) refidx = n;
            if (refidx < 1 || refidx > n) return fail(ctx, POLEE_ERR_BAD_ARG, "refidx %d is not in 1..%d", refidx, n);
            ref = refidx - 1;
        } else {
            ref = n - 1;  // xs[n] = 1 (:124)
        }
        nblk = (int)std::min<int64_t>(ceil_div((int64_t)n, ALT_THREADS), ALT_MAX_BLOCKS);
        const size_t nm1 = (size_t)n - 1;
        POLEE_TRY(d_mu.alloc(ctx, nm1));
        POLEE_TRY(d_omega.alloc(ctx, nm1));
        POLEE_TRY(d_z.alloc(ctx, nm1 * K));
        POLEE_TRY(d_x.alloc(ctx, (size_t)n * K));
        POLEE_TRY(d_part_stats.alloc(ctx, (size_t)K * nblk * 2));
        POLEE_TRY(d_part_apply.alloc(ctx, (size_t)K * nblk * 3));
        POLEE_TRY(d_ms.alloc(ctx, (size_t)K * 2));
        if (method == POLEE_ALT_NORMAL_ILR) {
            const PttPlan &pl = t->plans[0];
            std::vector<int32_t> r(nm1), s(nm1);
            for (size_t k = 0; k < nm1; ++k) {
                r[k] = pl.hi1[k] - pl.mid[k];  // leaves of the left child
                s[k] = pl.mid[k] - pl.lo[k];   // leaves of the right child
            }
            std::vector<double> ab(nm1 * 2);
            POLEE_TRY(polee_ilr_coefficients(r.data(), s.data(), (int64_t)nm1, ab.data()));
            POLEE_TRY(d_ab.upload(ctx, ab));
            POLEE_TRY(d_eta.alloc(ctx, (size_t)n * K));
            POLEE_TRY(d_chunk.alloc(ctx, (size_t)K * std::max(scan_num_chunks(3 * (int64_t)n - 2), 1)));
            ptt_retain(t);
            tree_retained = true;
        }
        return POLEE_OK;
    }
    void drop()
    {
        if (tree_retained) ptt_release(t);
        tree_retained = false;
        t = nullptr;
    }
    AltEta eta(const float *z) const
    {
        const bool ilr = method == POLEE_ALT_NORMAL_ILR;
        return AltEta{ilr ? d_eta.p : nullptr, ilr ? t->d_leaf_tid.p : nullptr, d_mu.p, d_omega.p, z, n, ref};
    }
    // xs of the K draws with noise z, into d_x [n][K]; g (optional) is zeroed; the side sums land in d_part_apply
    polee_status forward(const float *z, float *g)
    {
        hipStream_t st = ctx->stream;
        const AltEta e = eta(z);
        if (method == POLEE_ALT_NORMAL_ILR) {
            AltEta ey = e;
            ey.eta = nullptr;
            const AltTourLoad ld{t->view(), ey, d_ab.p};
            POLEE_HIP_TRY(ctx, run_scan<double>(st, K, t->TL, d_chunk.p, ld, AltTourEmit{ld, d_eta.p}));
        }
        hipLaunchKernelGGL(alt_softmax_stats_kernel, dim3(nblk, K), dim3(ALT_THREADS), 0, st, e, d_part_stats.p);
        hipLaunchKernelGGL(alt_softmax_finish_kernel, dim3(1), dim3(64 * K), 0, st, (const double *)d_part_stats.p, nblk, (int)K, d_ms.p);
        hipLaunchKernelGGL(alt_softmax_apply_kernel, dim3(nblk, K), dim3(ALT_THREADS), 0, st, e, (const double *)d_ms.p, (int)K, (float)eps,
                           (float)(1.0 - eps), d_x.p, g, d_part_apply.p);
        POLEE_KERNEL_CHECK(ctx);
        return POLEE_OK;
    }
};

}  // namespace polee

using namespace polee;

struct polee_altvi {
    polee_ctx *ctx = nullptr;
    polee_loglik *ll = nullptr;
    polee_altvi_opts o;
    AltCore core;
    int32_t n = 0, K = 0, step = 0, z_step = 0, trace_cap = 0;
    DevBuf<float> d_m0, d_v0, d_m1, d_v1, d_z0, d_g, d_mug, d_omg, d_x_rows;
    DevBuf<double> d_part_dot, d_st, d_P, d_lp, d_elbo, d_lptrace, d_ygrad, d_xgrad_rows;
    DevBuf<int> d_flag;

    polee_status one_step(bool apply, bool want_values, bool hook);
};

polee_status polee_altvi::one_step(bool apply, bool want_values, bool hook)
{
    const int step_num = step + 1;
    const int64_t nm1 = (int64_t)n - 1;
    hipStream_t st = ctx->stream;
    if (o.z0 && step_num > o.num_steps) return fail(ctx, POLEE_ERR_BAD_ARG, "caller-supplied z0 covers only %d steps", o.num_steps);
    const float *z;
    if (o.z0) {
        z = d_z0.p + (size_t)(step_num - 1) * K * nm1;
    } else {
        if (z_step != step_num) {
            hipLaunchKernelGGL(alt_noise_kernel, dim3((unsigned)ceil_div(nm1, 256), K), dim3(256), 0, st, o.seed, step_num, nm1, core.d_z.p);
            z_step = step_num;
        }
        z = core.d_z.p;
    }
    const bool ilr = core.method == POLEE_ALT_NORMAL_ILR;
    POLEE_TRY(core.forward(z, d_g.p));
    if (want_values) POLEE_HIP_TRY(ctx, hipMemsetAsync(d_lp.p, 0, sizeof(double) * PSELL_MAX_K, st));
    POLEE_TRY(loglik_eval_device(ll, core.d_x.p, K, d_g.p, want_values ? d_lp.p : nullptr));
    const int nblk = core.nblk;
    hipLaunchKernelGGL(alt_dot_kernel, dim3(nblk, K), dim3(ALT_THREADS), 0, st, (const float *)core.d_x.p, (const float *)d_g.p, (int)K, (int64_t)n,
                       ilr ? 1 : 0, d_part_dot.p);
    hipLaunchKernelGGL(alt_draw_finish_kernel, dim3(1), dim3(64 * K), 0, st, core.method, (const double *)core.d_part_apply.p,
                       (const double *)d_part_dot.p, (const double *)core.d_ms.p, nblk, (int)K, (int64_t)n, d_st.p);
    POLEE_KERNEL_CHECK(ctx);
    const AltEta e = core.eta(z);
    if (ilr) {
        const AltLeafGradLoad ld{e, core.d_ms.p, d_st.p, core.d_x.p, d_g.p, (int)K};
        POLEE_HIP_TRY(ctx, run_scan<double>(st, K, (int64_t)n, core.d_chunk.p, ld, AltPrefixEmit{(int64_t)n, d_P.p}));
    }
    AdamConsts a = adam_schedule(o, step_num);
    a.max_mu = o.max_step0;
    a.max_omega = o.max_step1;
    const bool noise_next = apply && !o.z0;
    AltUpd u;
    u.method = core.method;
    u.K = K;
    u.apply = apply ? 1 : 0;
    u.step = step_num;
    u.n = n;
    u.e = e;
    u.x = core.d_x.p;
    u.g = d_g.p;
    u.st = d_st.p;
    u.P = d_P.p;
    u.ab = core.d_ab.p;
    u.lo = ilr ? core.t->d_lo.p : nullptr;
    u.mid = ilr ? core.t->d_mid.p : nullptr;
    u.hi1 = ilr ? core.t->d_hi1.p : nullptr;
    u.mu = core.d_mu.p;
    u.omega = core.d_omega.p;
    u.m0 = d_m0.p;
    u.v0 = d_v0.p;
    u.m1 = d_m1.p;
    u.v1 = d_v1.p;
    u.adam = a;
    u.flag = d_flag.p;
    u.ygrad = hook ? d_ygrad.p : nullptr;
    u.mug = hook ? d_mug.p : nullptr;
    u.omg = hook ? d_omg.p : nullptr;
    u.znext = noise_next ? core.d_z.p : nullptr;
    u.seed = o.seed;
    hipLaunchKernelGGL(alt_update_kernel, dim3((unsigned)ceil_div(nm1, ALT_THREADS)), dim3(ALT_THREADS), 0, st, u);
    if (noise_next) z_step = step_num + 1;
    if (want_values && apply && step < trace_cap)
        hipLaunchKernelGGL(alt_trace_kernel, dim3(1), dim3(64), 0, st, core.method, (const double *)d_lp.p, (const double *)d_st.p, (int)K, step,
                           d_elbo.p, d_lptrace.p);
    POLEE_KERNEL_CHECK(ctx);
    if (apply) ++step;
    return POLEE_OK;
}

extern "C" {

polee_status polee_altvi_create(polee_loglik *ll, polee_ptt *t, const polee_altvi_opts *opts, polee_altvi **out)
{
    return entry(ll, "polee_altvi_create", [&](polee_ctx *ctx) -> polee_status {
        if (!out || !opts) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_altvi_create: null argument");
        if (opts->num_steps < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "num_steps must be >= 0");
        if (!(opts->eps > 0.0 && opts->eps < 0.5)) return fail(ctx, POLEE_ERR_BAD_ARG, "eps must lie in (0, 0.5)");
        if (ll->n > INT32_MAX) return fail(ctx, POLEE_ERR_UNSUPPORTED, "too many transcripts");
        polee_altvi *A = new (std::nothrow) polee_altvi();
        if (!A) return fail(ctx, POLEE_ERR_OOM, "out of host memory");
        A->ctx = ctx;
        A->ll = ll;
        ctx_retain(ctx);
        loglik_retain(ll);
        A->o = *opts;
        A->n = (int32_t)ll->n;
        A->K = opts->num_mc_samples;
        A->core.eps = opts->eps;
        auto bail = [&](polee_status s) {
            polee_altvi_destroy(A);
            return s;
        };
        polee_status s;
        if ((s = A->core.init(ctx, opts->method, t, A->n, A->K, opts->refidx))) return bail(s);
        const size_t n = (size_t)A->n, nm1 = n - 1, K = (size_t)A->K;
        for (DevBuf<float> *b : {&A->d_m0, &A->d_v0, &A->d_m1, &A->d_v1, &A->d_mug, &A->d_omg})
            if ((s = b->alloc(ctx, nm1))) return bail(s);
        if ((s = A->d_g.alloc(ctx, n * K)) || (s = A->d_x_rows.alloc(ctx, n * K)) || (s = A->d_xgrad_rows.alloc(ctx, n * K)) ||
            (s = A->d_ygrad.alloc(ctx, nm1 * K)) || (s = A->d_part_dot.alloc(ctx, K * A->core.nblk)) || (s = A->d_st.alloc(ctx, K * 4)) ||
            (s = A->d_lp.alloc(ctx, PSELL_MAX_K)) || (s = A->d_flag.alloc(ctx, 1)))
            return bail(s);
        if (A->core.method == POLEE_ALT_NORMAL_ILR && (s = A->d_P.alloc(ctx, (n + 1) * K))) return bail(s);
        A->trace_cap = opts->gradonly ? 0 : std::max(opts->num_steps, 1);
        if (!opts->gradonly && ((s = A->d_elbo.alloc(ctx, A->trace_cap)) || (s = A->d_lptrace.alloc(ctx, A->trace_cap)))) return bail(s);
        if (opts->z0 && opts->num_steps > 0 && (s = A->d_z0.upload(ctx, opts->z0, (size_t)opts->num_steps * K * nm1))) return bail(s);
        // initial values: mu = 0; omega = 0.1 for the logistic-normal (:79, not log 0.1), log(0.1f0) for ILR and ALR (:536, 655)
        std::vector<float> mu(nm1, 0.0f), om(nm1, A->core.method == POLEE_ALT_LOGISTIC_NORMAL ? 0.1f : logf(0.1f));
        if ((s = A->core.d_mu.upload(ctx, mu)) || (s = A->core.d_omega.upload(ctx, om))) return bail(s);
        hipError_t e = hipMemsetAsync(A->d_flag.p, 0, sizeof(int), ctx->stream);
        for (DevBuf<float> *b : {&A->d_m0, &A->d_v0, &A->d_m1, &A->d_v1})
            if (e == hipSuccess) e = hipMemsetAsync(b->p, 0, sizeof(float) * nm1, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return bail(fail(ctx, POLEE_ERR_HIP, "polee_altvi_create: %s", hipGetErrorString(e)));
        *out = A;
        return POLEE_OK;
    });
}

void polee_altvi_destroy(polee_altvi *A)
{
    if (!A) return;
    polee_ctx *ctx = A->ctx;
    polee_loglik *ll = A->ll;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    A->core.drop();
    delete A;
    loglik_release(ll);
    ctx_release(ctx);
}

polee_status polee_altvi_run(polee_altvi *A, int32_t nsteps)
{
    return entry(A, "polee_altvi_run", [&](polee_ctx *ctx) -> polee_status {
        for (int32_t i = 0; i < nsteps; ++i) POLEE_TRY(A->one_step(true, !A->o.gradonly, false));
        return POLEE_OK;
    });
}

polee_status polee_altvi_sync(polee_altvi *A)
{
    return entry(A, "polee_altvi_sync", [&](polee_ctx *ctx) -> polee_status {
        int flag = 0;
        POLEE_TRY(A->d_flag.download(ctx, &flag, 1));
        if (flag != 0) return fail(ctx, POLEE_ERR_NONFINITE, "non-finite gradient at step %d of the alternative approximation", flag);
        return POLEE_OK;
    });
}

polee_status polee_altvi_get_params(polee_altvi *A, float *p0, float *p1)
{
    return entry(A, "polee_altvi_get_params", [&](polee_ctx *ctx) -> polee_status {
        if (p0) POLEE_TRY(A->core.d_mu.download(ctx, p0, (size_t)A->n - 1));
        if (p1) POLEE_TRY(A->core.d_omega.download(ctx, p1, (size_t)A->n - 1));
        return POLEE_OK;
    });
}

polee_status polee_altvi_set_params(polee_altvi *A, const float *p0, const float *p1)
{
    return entry(A, "polee_altvi_set_params", [&](polee_ctx *ctx) -> polee_status {
        if (p0) POLEE_TRY(A->core.d_mu.upload(ctx, p0, (size_t)A->n - 1));
        if (p1) POLEE_TRY(A->core.d_omega.upload(ctx, p1, (size_t)A->n - 1));
        return POLEE_OK;
    });
}

polee_status polee_altvi_get_stats(polee_altvi *A, polee_altvi_stats *stats)
{
    return entry(A, "polee_altvi_get_stats", [&](polee_ctx *ctx) -> polee_status {
        if (!stats) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_altvi_get_stats: null argument");
        memset(stats, 0, sizeof(*stats));
        stats->steps_done = A->step;
        POLEE_TRY(A->d_flag.download(ctx, &stats->nonfinite_step, 1));
        if (!A->o.gradonly && A->step > 0 && A->step <= A->trace_cap) {
            POLEE_HIP_TRY(ctx, hipMemcpy(&stats->last_elbo, A->d_elbo.p + (A->step - 1), sizeof(double), hipMemcpyDeviceToHost));
            POLEE_HIP_TRY(ctx, hipMemcpy(&stats->last_lp_mean, A->d_lptrace.p + (A->step - 1), sizeof(double), hipMemcpyDeviceToHost));
        }
        return POLEE_OK;
    });
}

polee_status polee_altvi_get_trace(polee_altvi *A, double *elbo, double *lp_mean)
{
    return entry(A, "polee_altvi_get_trace", [&](polee_ctx *ctx) -> polee_status {
        if (A->o.gradonly) return fail(ctx, POLEE_ERR_BAD_ARG, "no trace is recorded in gradonly mode");
        const size_t cnt = (size_t)std::min(A->step, A->trace_cap);
        if (elbo) POLEE_TRY(A->d_elbo.download(ctx, elbo, cnt));
        if (lp_mean) POLEE_TRY(A->d_lptrace.download(ctx, lp_mean, cnt));
        return POLEE_OK;
    });
}

polee_status polee_altvi_export_noise(polee_altvi *A, int32_t step, float *z0)
{
    return entry(A, "polee_altvi_export_noise", [&](polee_ctx *ctx) -> polee_status {
        if (!z0 || step < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_altvi_export_noise: bad argument");
        const int64_t nm1 = (int64_t)A->n - 1;
        const size_t cnt = (size_t)A->K * nm1;
        if (A->o.z0) {
            if (step > A->o.num_steps) return fail(ctx, POLEE_ERR_BAD_ARG, "step beyond the supplied noise");
            POLEE_HIP_TRY(ctx, hipMemcpyAsync(z0, A->d_z0.p + (size_t)(step - 1) * cnt, cnt * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return POLEE_OK;
        }
        DevBuf<float> tmp;
        POLEE_TRY(tmp.alloc(ctx, cnt));
        hipLaunchKernelGGL(alt_noise_kernel, dim3((unsigned)ceil_div(nm1, 256), A->K), dim3(256), 0, ctx->stream, A->o.seed, (int)step, nm1, tmp.p);
        POLEE_KERNEL_CHECK(ctx);
        return tmp.download(ctx, z0, cnt);
    });
}

polee_status polee_altvi_eval_gradients(polee_altvi *A, float *xs, double *x_grad, double *y_grad, float *p0_grad, float *p1_grad, double *lp,
                                        double *ladj)
{
    return entry(A, "polee_altvi_eval_gradients", [&](polee_ctx *ctx) -> polee_status {
        const size_t n = (size_t)A->n, nm1 = n - 1, K = (size_t)A->K;
        POLEE_TRY(A->one_step(false, true, true));
        const unsigned nb = (unsigned)ceil_div((int64_t)(n * K), 256);
        hipLaunchKernelGGL(alt_rows_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const float *)A->core.d_x.p, (int)K, (int64_t)n, A->d_x_rows.p,
                           (double *)nullptr);
        hipLaunchKernelGGL(alt_rows_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const float *)A->d_g.p, (int)K, (int64_t)n, (float *)nullptr,
                           A->d_xgrad_rows.p);
        POLEE_KERNEL_CHECK(ctx);
        if (xs) POLEE_TRY(A->d_x_rows.download(ctx, xs, n * K));
        if (x_grad) POLEE_TRY(A->d_xgrad_rows.download(ctx, x_grad, n * K));
        if (y_grad) POLEE_TRY(A->d_ygrad.download(ctx, y_grad, nm1 * K));
        if (p0_grad) POLEE_TRY(A->d_mug.download(ctx, p0_grad, nm1));
        if (p1_grad) POLEE_TRY(A->d_omg.download(ctx, p1_grad, nm1));
        if (lp) POLEE_TRY(A->d_lp.download(ctx, lp, K));
        if (ladj) {
            std::vector<double> st(K * 4);
            POLEE_TRY(A->d_st.download(ctx, st.data(), K * 4));
            for (size_t d = 0; d < K; ++d) ladj[d] = st[d * 4 + 2];
        }
        return POLEE_OK;
    });
}

polee_status polee_alt_sample(polee_ctx *ctx, int32_t method, polee_ptt *t, int32_t n, const float *p0, const float *p1, const float *efflens,
                              int32_t refidx, int32_t count, uint64_t seed, const float *z0, float *out)
{
    return ctx_entry(ctx, "polee_alt_sample", [&]() -> polee_status {
        if (!p0 || !p1 || !efflens || !out || count < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_alt_sample: bad argument");
        const int32_t B = std::min<int32_t>(count, PSELL_MAX_K);
        AltCore core;
        polee_status s = core.init(ctx, method, t, n, B, refidx);
        if (s != POLEE_OK) {
            core.drop();
            return s;
        }
        const size_t nm1 = (size_t)n - 1;
        DevBuf<float> d_eff, d_out;
        DevBuf<double> d_part;
        auto body = [&]() -> polee_status {
            POLEE_TRY(core.d_mu.upload(ctx, p0, nm1));
            POLEE_TRY(core.d_omega.upload(ctx, p1, nm1));
            POLEE_TRY(d_eff.upload(ctx, efflens, (size_t)n));
            POLEE_TRY(d_out.alloc(ctx, (size_t)B * n));
            POLEE_TRY(d_part.alloc(ctx, (size_t)B * core.nblk));
            for (int32_t b0 = 0; b0 < count; b0 += B) {
                const int32_t R = std::min(B, count - b0);
                // (a short last batch runs B rows as well: the rows past R draw noise of their own and are not copied out)
                if (z0) {
                    POLEE_HIP_TRY(ctx, hipMemsetAsync(core.d_z.p, 0, sizeof(float) * nm1 * B, ctx->stream));
                    POLEE_TRY(core.d_z.upload(ctx, z0 + (size_t)b0 * nm1, (size_t)R * nm1));
                } else {
                    hipLaunchKernelGGL(alt_noise_kernel, dim3((unsigned)ceil_div((int64_t)nm1, 256), B), dim3(256), 0, ctx->stream, seed,
                                       b0 / B + 1, (int64_t)nm1, core.d_z.p);
                }
                POLEE_TRY(core.forward(core.d_z.p, nullptr));
                hipLaunchKernelGGL(alt_sample_sum_kernel, dim3(core.nblk, B), dim3(ALT_THREADS), 0, ctx->stream, (const float *)core.d_x.p,
                                   (const float *)d_eff.p, (int)B, (int64_t)n, d_part.p);
                hipLaunchKernelGGL(alt_sample_write_kernel, dim3((unsigned)ceil_div((int64_t)n, 256), B), dim3(256), 0, ctx->stream,
                                   (const float *)core.d_x.p, (const float *)d_eff.p, (const double *)d_part.p, core.nblk, (int)B, (int64_t)n, d_out.p);
                POLEE_KERNEL_CHECK(ctx);
                POLEE_TRY(d_out.download(ctx, out + (size_t)b0 * n, (size_t)R * n));
            }
            return POLEE_OK;
        };
        s = body();
        (void)hipStreamSynchronize(ctx->stream);
        core.drop();
        return s;
    });
}

}  // extern "C"

// `polee sample` (src/main.jl:756-919) on the device: a streaming handle over the sampler's draws -- effective-length adjustment,
// running posterior mean, prop_to_counts -- and an exact multinomial sampler for --sample-counts.
//
// The reference draws the m reads of a bootstrap one by one through a binary search (main.jl:865-874).  Here a draw's counts come
// from n - 1 binomial variates, whatever m is: the count m at the root of a balanced binary tree over the categories is split
// level by level, a node covering [lo, hi) with count c handing Binomial(c, mass[lo, mid) / mass[lo, hi)) to its left half and the
// rest to its right half.  The masses are differences of a double-double prefix sum of the shares (scan.hpp), the variates are
// binomial.hpp's, keyed by (seed, draw index, node): a row of counts is a pure function of (shares, m, seed, draw index).  No
// atomics anywhere in this file.  Launch shape and resource usage: DESIGN.md §3.9.
#include "binomial.hpp"
#include "common.hpp"
#include "ptt_internal.hpp"
#include "sampler_internal.hpp"
#include "scan.hpp"
#include "../../include/polee_hip_debug.h"

#include <cmath>

namespace polee {
namespace {

// ---- exact multinomial ------------------------------------------------------------------------------------------------------

constexpr int MN_TOP_LEVELS = 8;      // levels 0..7 (at most 128 nodes) run in one workgroup per row; the wider ones one launch each
constexpr int64_t MN_MAX_N = (int64_t)1 << 30;
constexpr int64_t MN_CHUNK_ELEMS = (int64_t)1 << 22;  // rows of a call are processed in groups of about this many shares

struct MnArgs {
    const dd *P;  // [R][n + 1] prefix of the shares: P[0] = 0, P[j + 1] = p_0 + ... + p_j
    int64_t n;
    int L;  // ceil(log2 n): level L has 2^L nodes covering at most one category each
    int64_t m;
    uint64_t seed, first_draw;  // row r is draw first_draw + r
    uint32_t *counts;           // [R][n]
    int *err;
};

// Node i of level lev covers [i n / 2^lev, (i + 1) n / 2^lev) (floors); its children are nodes 2i and 2i + 1 of level lev + 1.
__device__ inline void mn_split(const MnArgs &a, int row, int lev, uint32_t i, uint32_t c, uint32_t *left, uint32_t *right)
{
    uint32_t l = 0;
    if (c > 0) {
        const int64_t lo = ((int64_t)i * a.n) >> lev, hi = ((int64_t)(i + 1) * a.n) >> lev;
        const int64_t mid = ((int64_t)(2 * (int64_t)i + 1) * a.n) >> (lev + 1);
        if (mid <= lo) {
            l = 0;
        } else if (hi <= mid) {
            l = c;
        } else {
            const dd *P = a.P + (int64_t)row * (a.n + 1);
            const double wl = dd_diff(P[mid], P[lo]), wr = dd_diff(P[hi], P[mid]);
            const double w = wl + wr;
            const uint64_t draw = a.first_draw + (uint64_t)row;
            const uint32_t node = ((uint32_t)1 << lev) + i;
            int bad = 0;
            if (!(w > 0.0)) l = 0;  // (a node without mass holds no count below a root that has some)
            else if (wl <= wr) l = (uint32_t)binomial_draw((int64_t)c, wl / w, a.seed, draw, node, &bad);
            else l = c - (uint32_t)binomial_draw((int64_t)c, wr / w, a.seed, draw, node, &bad);
            if (bad) *a.err = 1;
        }
    }
    *left = l;
    *right = c - l;
}

// the count of node i of the last level goes to the category it covers, if any
__device__ inline void mn_store_leaf(const MnArgs &a, int row, uint32_t i, uint32_t c)
{
    const int64_t lo = ((int64_t)i * a.n) >> a.L, hi = ((int64_t)(i + 1) * a.n) >> a.L;
    if (hi > lo) a.counts[(int64_t)row * a.n + lo] = c;
}

// levels 0 .. Ltop-1 of one row in LDS; the 2^Ltop counts of level Ltop go to `out` [R][2^Ltop], or to the categories when Ltop == L
__global__ __launch_bounds__(256) void mn_top_kernel(MnArgs a, int Ltop, uint32_t *out)
{
    __shared__ uint32_t s[2][256];
    const int row = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s[0][0] = (uint32_t)a.m;
    __syncthreads();
    int cur = 0;
    for (int lev = 0; lev < Ltop; ++lev) {
        if (tid < ((uint32_t)1 << lev)) {
            uint32_t l, r;
            mn_split(a, row, lev, tid, s[cur][tid], &l, &r);
            s[cur ^ 1][2 * tid] = l;
            s[cur ^ 1][2 * tid + 1] = r;
        }
        __syncthreads();
        cur ^= 1;
    }
    const uint32_t W = (uint32_t)1 << Ltop;
    if (tid < W) {
        if (Ltop == a.L) mn_store_leaf(a, row, tid, s[cur][tid]);
        else out[(int64_t)row * W + tid] = s[cur][tid];
    }
}

// one level: in [R][2^lev] -> out [R][2^(lev+1)], or the categories when lev + 1 == L
__global__ __launch_bounds__(256) void mn_level_kernel(MnArgs a, int lev, const uint32_t *in, uint32_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    const int64_t W = (int64_t)1 << lev;
    if (i >= W) return;
    uint32_t l, r;
    mn_split(a, row, lev, (uint32_t)i, in[(int64_t)row * W + i], &l, &r);
    if (lev + 1 == a.L) {
        mn_store_leaf(a, row, (uint32_t)(2 * i), l);
        mn_store_leaf(a, row, (uint32_t)(2 * i + 1), r);
    } else {
        out[(int64_t)row * 2 * W + 2 * i] = l;
        out[(int64_t)row * 2 * W + 2 * i + 1] = r;
    }
}

struct ShareLoad {
    const double *p;
    int64_t n;
    __device__ dd operator()(int row, int64_t idx) const { return dd_make(p[(int64_t)row * n + idx]); }
};
struct PrefixEmit {
    dd *P;
    int64_t n;
    __device__ void operator()(int row, int64_t idx, dd, dd inclusive) const
    {
        dd *r = P + (int64_t)row * (n + 1);
        if (idx == 0) r[0] = dd{0.0, 0.0};
        r[idx + 1] = inclusive;
    }
};

// any share that is negative or not finite raises the flag (every thread that finds one stores the same value)
__global__ void mn_check_kernel(const double *p, int64_t count, int *flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && !(p[i] >= 0.0 && p[i] <= 1.7976931348623157e308)) *flag = 1;
}
__global__ void mn_totals_kernel(const dd *P, int64_t n, int R, double *totals)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) totals[r] = P[(int64_t)r * (n + 1) + n].hi;
}

inline int mn_levels(int64_t n)
{
    int L = 0;
    while (((int64_t)1 << L) < n) ++L;
    return L;
}

struct MnWork {
    DevBuf<dd> P, chunk;
    DevBuf<uint32_t> a, b;
    polee_status reserve(polee_ctx *ctx, int R, int64_t n)
    {
        const int L = mn_levels(n);
        const size_t half = (size_t)1 << std::max(L - 1, 8);
        POLEE_TRY(P.alloc(ctx, (size_t)R * (size_t)(n + 1)));
        POLEE_TRY(chunk.alloc(ctx, (size_t)R * (size_t)std::max(scan_num_chunks(n), 1)));
        POLEE_TRY(a.alloc(ctx, (size_t)R * half));
        POLEE_TRY(b.alloc(ctx, (size_t)R * half));
        return POLEE_OK;
    }
};

// the prefix of R rows of shares (device, f64 [R][n]); queued
polee_status mn_prefix_device(polee_ctx *ctx, MnWork &w, const double *d_p, int R, int64_t n)
{
    POLEE_TRY(w.reserve(ctx, R, n));
    hipError_t e = run_scan<dd>(ctx->stream, R, n, w.chunk.p, ShareLoad{d_p, n}, PrefixEmit{w.P.p, n});
    if (e != hipSuccess) return fail(ctx, POLEE_ERR_HIP, "prefix scan launch failed: %s", hipGetErrorString(e));
    return POLEE_OK;
}

// R rows of counts from the prefix in w.P (rows are draws first_draw, first_draw + 1, ...); queued, no synchronisation
polee_status mn_split_device(polee_ctx *ctx, MnWork &w, int R, int64_t n, int64_t m, uint64_t seed, uint64_t first_draw,
                             uint32_t *d_counts, int *d_err)
{
    MnArgs a{w.P.p, n, mn_levels(n), m, seed, first_draw, d_counts, d_err};
    const int Ltop = std::min(a.L, MN_TOP_LEVELS);
    hipLaunchKernelGGL(mn_top_kernel, dim3((unsigned)R), dim3(256), 0, ctx->stream, a, Ltop, w.a.p);
    POLEE_KERNEL_CHECK(ctx);
    uint32_t *in = w.a.p, *out = w.b.p;
    for (int lev = Ltop; lev < a.L; ++lev) {
        hipLaunchKernelGGL(mn_level_kernel, dim3((unsigned)ceil_div((int64_t)1 << lev, 256), (unsigned)R), dim3(256), 0, ctx->stream,
                           a, lev, (const uint32_t *)in, out);
        POLEE_KERNEL_CHECK(ctx);
        std::swap(in, out);
    }
    return POLEE_OK;
}

inline int mn_rows_per_group(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(1024, MN_CHUNK_ELEMS / std::max<int64_t>(n, 1))); }

__global__ void debug_binomial_kernel(const int64_t *N, const double *p, int64_t count, uint64_t seed, int64_t *out, int *err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    int bad = 0;
    out[i] = binomial_draw(N[i], p[i], seed, (uint64_t)i, 0u, &bad);
    if (bad) *err = 1;
}

// ---- the streaming handle's kernels ---------------------------------------------------------------------------------------------

constexpr int SM_ROW_THREADS = 1024;

// block-wide f64 sum in a fixed order, handed to every thread (smem: one double per wave + 1)
__device__ inline double sm_block_sum(double v, double *smem)
{
    v = wave_inclusive_scan<double>(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 63) smem[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int w = 0; w < nw; ++w) r += smem[w];
        smem[nw] = r;
    }
    __syncthreads();
    const double r = smem[nw];
    __syncthreads();
    return r;
}

// per draw (one workgroup each): S = sum_j x_j / l_j and, with prop_j = (float)((x_j / l_j) / S), E = sum_j prop_j l_j; both in f64
__global__ __launch_bounds__(SM_ROW_THREADS) void sm_row_sums_kernel(const float *xs, const float *l, int64_t n, double *S, double *E)
{
    __shared__ double smem[SM_ROW_THREADS / 64 + 1];
    const float *x = xs + (int64_t)blockIdx.x * n;
    double q = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += blockDim.x) q += (double)(x[j] / l[j]);
    const double s = sm_block_sum(q, smem);
    double e = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += blockDim.x) {
        const float prop = (float)((double)(x[j] / l[j]) / s);
        e += (double)prop * (double)l[j];
    }
    e = sm_block_sum(e, smem);
    if (threadIdx.x == 0) {
        S[blockIdx.x] = s;
        E[blockIdx.x] = e;
    }
}

// thread per transcript over the B draws of a block, in draw order: props, expected counts or the shares the multinomial splits,
// and the posterior mean's f64 accumulator
__global__ void sm_emit_kernel(const float *xs, const float *l, const double *S, const double *E, int B, int64_t n, double m,
                               float *props, double *counts, double *shares, double *acc)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const float lj = l[j];
    double sum = acc[j];
    for (int d = 0; d < B; ++d) {
        const float prop = (float)((double)(xs[(int64_t)d * n + j] / lj) / S[d]);
        sum += (double)prop;
        const double e = (double)prop * (double)lj;
        if (props) props[(int64_t)d * n + j] = prop;
        if (counts) counts[(int64_t)d * n + j] = e / E[d] * m;
        if (shares) shares[(int64_t)d * n + j] = e;
    }
    acc[j] = sum;
}

__global__ void sm_counts_to_f64_kernel(const uint32_t *c, int64_t count, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = (double)c[i];
}

// post_mean = (float)(acc / ndraws) and prop_to_counts of it (one workgroup): expected counts, or the shares for the multinomial
__global__ __launch_bounds__(SM_ROW_THREADS) void sm_mean_kernel(const double *acc, const float *l, int64_t n, double ndraws, double m,
                                                                 float *pm, double *counts, double *shares)
{
    __shared__ double smem[SM_ROW_THREADS / 64 + 1];
    double e = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += blockDim.x) {
        const float v = (float)(acc[j] / ndraws);
        pm[j] = v;
        e += (double)v * (double)l[j];
    }
    e = sm_block_sum(e, smem);
    for (int64_t j = threadIdx.x; j < n; j += blockDim.x) {
        const double ej = (double)pm[j] * (double)l[j];
        if (counts) counts[j] = ej / e * m;
        if (shares) shares[j] = ej;
    }
}

polee_status check_attempts(polee_ctx *ctx, DevBuf<int> &d_err, const char *what)
{
    int bad = 0;
    POLEE_TRY(d_err.download(ctx, &bad, 1));
    if (bad) {
        POLEE_HIP_TRY(ctx, hipMemsetAsync(d_err.p, 0, sizeof(int), ctx->stream));
        return fail(ctx, POLEE_ERR_NONFINITE, "%s: a binomial variate used up its %d attempts (non-finite shares?)", what,
                    BINOMIAL_MAX_ATTEMPTS);
    }
    return POLEE_OK;
}

}  // namespace
}  // namespace polee

using namespace polee;

struct polee_sampler {
    polee_ctx *ctx = nullptr;
    polee_ptt *t = nullptr;
    int64_t n = 0, m = 0;
    uint64_t seed = 0;
    uint64_t next_draw = 0;  // draws made so far = the index of the next one
    DevBuf<float> d_mu, d_sigma, d_alpha, d_l, d_z0, d_raw, d_props, d_pm;
    DevBuf<double> d_acc, d_S, d_E, d_shares, d_counts;
    DevBuf<uint32_t> d_cnt;
    DevBuf<int> d_err;
    MnWork mn;
};

extern "C" {

polee_status polee_sampler_create(polee_ptt *t, const float *mu, const float *sigma, const float *alpha, const float *efflens,
                                  int64_t m, uint64_t seed, polee_sampler **out)
{
    return entry(t, "polee_sampler_create", [&](polee_ctx *ctx) -> polee_status {
        if (!out || !mu || !sigma || !alpha || !efflens) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_create: null argument");
        if (t->T != 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_create: the sampler needs a single tree");
        if (m < 0 || m >= ((int64_t)1 << 31))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_create: m = %lld outside [0, 2^31)", (long long)m);
        const int64_t n = t->n;
        if (n < 1 || n > MN_MAX_N) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_create: n = %lld outside [1, 2^30]", (long long)n);
        for (int64_t j = 0; j < n; ++j)
            if (!(efflens[j] > 0.0f && efflens[j] <= 3.4028234e38f))
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_create: effective length %lld is not a positive finite number",
                            (long long)j);
        polee_sampler *s = new (std::nothrow) polee_sampler();
        if (!s) return fail(ctx, POLEE_ERR_OOM, "out of host memory");
        s->ctx = ctx;
        ctx_retain(ctx);
        s->t = t;
        ptt_retain(t);
        s->n = n;
        s->m = m;
        s->seed = seed;
        const size_t nm1 = (size_t)n - 1;
        polee_status st;
        if ((st = s->d_mu.upload(ctx, mu, nm1)) || (st = s->d_sigma.upload(ctx, sigma, nm1)) || (st = s->d_alpha.upload(ctx, alpha, nm1)) ||
            (st = s->d_l.upload(ctx, efflens, (size_t)n)) || (st = s->d_acc.alloc(ctx, (size_t)n)) || (st = s->d_pm.alloc(ctx, (size_t)n)) ||
            (st = s->d_S.alloc(ctx, SAMPLER_BLOCK)) || (st = s->d_E.alloc(ctx, SAMPLER_BLOCK)) || (st = s->d_err.alloc(ctx, 1))) {
            polee_sampler_destroy(s);
            return st;
        }
        hipError_t e = hipMemsetAsync(s->d_acc.p, 0, sizeof(double) * (size_t)n, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(s->d_err.p, 0, sizeof(int), ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            polee_sampler_destroy(s);
            return fail(ctx, POLEE_ERR_HIP, "polee_sampler_create: %s", hipGetErrorString(e));
        }
        *out = s;
        return POLEE_OK;
    });
}

void polee_sampler_destroy(polee_sampler *s)
{
    if (!s) return;
    polee_ctx *ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    polee_ptt *t = s->t;
    delete s;
    ptt_release(t);
    ctx_release(ctx);
}

polee_status polee_sampler_num_draws(polee_sampler *s, int64_t *ndraws)
{
    return entry(s, "polee_sampler_num_draws", [&](polee_ctx *ctx) -> polee_status {
        if (!ndraws) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_num_draws: null argument");
        *ndraws = (int64_t)s->next_draw;
        return POLEE_OK;
    });
}

polee_status polee_sampler_next(polee_sampler *s, int32_t count, int32_t count_mode, const float *z0_or_null, float *raw_or_null,
                                float *props_or_null, double *counts_or_null)
{
    return entry(s, "polee_sampler_next", [&](polee_ctx *ctx) -> polee_status {
        if (count < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_next: count < 1");
        if (count_mode != 0 && count_mode != 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_next: count_mode must be 0 or 1");
        const int64_t n = s->n;
        const size_t nm1 = (size_t)n - 1, total = (size_t)count * (size_t)n;
        const bool sampled = counts_or_null && count_mode == 1;
        POLEE_TRY(s->d_raw.alloc(ctx, total));
        if (props_or_null) POLEE_TRY(s->d_props.alloc(ctx, total));
        if (counts_or_null) POLEE_TRY(s->d_counts.alloc(ctx, total));
        if (sampled) {
            POLEE_TRY(s->d_shares.alloc(ctx, (size_t)SAMPLER_BLOCK * n));
            POLEE_TRY(s->d_cnt.alloc(ctx, (size_t)SAMPLER_BLOCK * n));
        }
        const uint64_t first = s->next_draw, end = first + (uint64_t)count;
        for (uint64_t d0 = first; d0 < end;) {
            const uint64_t b0 = d0 - d0 % SAMPLER_BLOCK;
            const int32_t r0 = (int32_t)(d0 - b0), B = (int32_t)(std::min<uint64_t>(end, b0 + SAMPLER_BLOCK) - d0);
            const size_t row = (size_t)(d0 - first);
            float *raw = s->d_raw.p + row * n;
            if (z0_or_null) POLEE_TRY(s->d_z0.upload(ctx, z0_or_null + row * nm1, (size_t)B * nm1));
            POLEE_TRY(sampler_block_device(s->t, s->d_mu.p, s->d_sigma.p, s->d_alpha.p, z0_or_null ? s->d_z0.p : nullptr, s->seed, b0, r0,
                                           B, 0.0, raw, n));
            hipLaunchKernelGGL(sm_row_sums_kernel, dim3((unsigned)B), dim3(SM_ROW_THREADS), 0, ctx->stream, (const float *)raw,
                               (const float *)s->d_l.p, n, s->d_S.p, s->d_E.p);
            hipLaunchKernelGGL(sm_emit_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream, (const float *)raw,
                               (const float *)s->d_l.p, (const double *)s->d_S.p, (const double *)s->d_E.p, (int)B, n, (double)s->m,
                               props_or_null ? s->d_props.p + row * n : (float *)nullptr,
                               counts_or_null && !sampled ? s->d_counts.p + row * n : (double *)nullptr,
                               sampled ? s->d_shares.p : (double *)nullptr, s->d_acc.p);
            POLEE_KERNEL_CHECK(ctx);
            if (sampled) {
                POLEE_TRY(mn_prefix_device(ctx, s->mn, s->d_shares.p, B, n));
                POLEE_TRY(mn_split_device(ctx, s->mn, B, n, s->m, s->seed, d0, s->d_cnt.p, s->d_err.p));
                hipLaunchKernelGGL(sm_counts_to_f64_kernel, dim3((unsigned)ceil_div((int64_t)B * n, 256)), dim3(256), 0, ctx->stream,
                                   (const uint32_t *)s->d_cnt.p, (int64_t)B * n, s->d_counts.p + row * n);
                POLEE_KERNEL_CHECK(ctx);
            }
            d0 += (uint64_t)B;
        }
        s->next_draw = end;
        if (raw_or_null) POLEE_TRY(s->d_raw.download(ctx, raw_or_null, total));
        if (props_or_null) POLEE_TRY(s->d_props.download(ctx, props_or_null, total));
        if (counts_or_null) POLEE_TRY(s->d_counts.download(ctx, counts_or_null, total));
        if (sampled) POLEE_TRY(check_attempts(ctx, s->d_err, "polee_sampler_next"));
        else POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (z0 is borrowed for the call only)
        return POLEE_OK;
    });
}

polee_status polee_sampler_mean(polee_sampler *s, float *post_mean, double *est_counts_or_null, int32_t count_mode)
{
    return entry(s, "polee_sampler_mean", [&](polee_ctx *ctx) -> polee_status {
        if (!post_mean) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_mean: null output");
        if (count_mode != 0 && count_mode != 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_mean: count_mode must be 0 or 1");
        if (s->next_draw == 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_sampler_mean: no draws yet");
        const int64_t n = s->n;
        const bool sampled = est_counts_or_null && count_mode == 1;
        if (est_counts_or_null) POLEE_TRY(s->d_counts.alloc(ctx, (size_t)n));
        if (sampled) {
            POLEE_TRY(s->d_shares.alloc(ctx, (size_t)n));
            POLEE_TRY(s->d_cnt.alloc(ctx, (size_t)n));
        }
        hipLaunchKernelGGL(sm_mean_kernel, dim3(1), dim3(SM_ROW_THREADS), 0, ctx->stream, (const double *)s->d_acc.p, (const float *)s->d_l.p,
                           n, (double)s->next_draw, (double)s->m, s->d_pm.p,
                           est_counts_or_null && !sampled ? s->d_counts.p : (double *)nullptr, sampled ? s->d_shares.p : (double *)nullptr);
        POLEE_KERNEL_CHECK(ctx);
        if (sampled) {
            // (the mean's counts are drawn under the draw index 2^64 - 1, which no draw of the stream reaches)
            POLEE_TRY(mn_prefix_device(ctx, s->mn, s->d_shares.p, 1, n));
            POLEE_TRY(mn_split_device(ctx, s->mn, 1, n, s->m, s->seed, ~(uint64_t)0, s->d_cnt.p, s->d_err.p));
            hipLaunchKernelGGL(sm_counts_to_f64_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, ctx->stream,
                               (const uint32_t *)s->d_cnt.p, n, s->d_counts.p);
            POLEE_KERNEL_CHECK(ctx);
        }
        POLEE_TRY(s->d_pm.download(ctx, post_mean, (size_t)n));
        if (est_counts_or_null) POLEE_TRY(s->d_counts.download(ctx, est_counts_or_null, (size_t)n));
        if (sampled) POLEE_TRY(check_attempts(ctx, s->d_err, "polee_sampler_mean"));
        return POLEE_OK;
    });
}

polee_status polee_multinomial_counts(polee_ctx *ctx, const double *p, int32_t D, int64_t n, int64_t m, uint64_t seed,
                                      uint64_t first_draw, uint32_t *counts)
{
    return ctx_entry(ctx, "polee_multinomial_counts", [&]() -> polee_status {
        if (!p || !counts) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_multinomial_counts: null argument");
        if (D < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_multinomial_counts: D < 1");
        if (n < 1 || n > MN_MAX_N) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_multinomial_counts: n = %lld outside [1, 2^30]", (long long)n);
        if (m < 0 || m >= ((int64_t)1 << 31))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_multinomial_counts: m = %lld outside [0, 2^31)", (long long)m);
        const int G = mn_rows_per_group(n);
        MnWork w;
        DevBuf<double> d_p, d_tot;
        DevBuf<uint32_t> d_cnt;
        DevBuf<int> d_flag;  // [0]: a bad share, [1]: attempts ran out
        POLEE_TRY(d_flag.alloc(ctx, 2));
        POLEE_TRY(d_tot.alloc(ctx, (size_t)G));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(d_flag.p, 0, 2 * sizeof(int), ctx->stream));
        std::vector<double> tot((size_t)G);
        for (int32_t r0 = 0; r0 < D; r0 += G) {
            const int R = std::min<int32_t>(G, D - r0);
            const int64_t cnt = (int64_t)R * n;
            POLEE_TRY(d_p.upload(ctx, p + (size_t)r0 * n, (size_t)cnt));
            POLEE_TRY(d_cnt.alloc(ctx, (size_t)cnt));
            hipLaunchKernelGGL(mn_check_kernel, dim3((unsigned)ceil_div(cnt, 256)), dim3(256), 0, ctx->stream, (const double *)d_p.p, cnt,
                               d_flag.p);
            POLEE_KERNEL_CHECK(ctx);
            POLEE_TRY(mn_prefix_device(ctx, w, d_p.p, R, n));
            hipLaunchKernelGGL(mn_totals_kernel, dim3((unsigned)ceil_div(R, 256)), dim3(256), 0, ctx->stream, (const dd *)w.P.p, n, R,
                               d_tot.p);
            POLEE_KERNEL_CHECK(ctx);
            int flag[2] = {0, 0};
            POLEE_TRY(d_flag.download(ctx, flag, 2));
            if (flag[0])
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_multinomial_counts: a share of rows %d..%d is negative or not finite", r0,
                            r0 + R - 1);
            POLEE_TRY(d_tot.download(ctx, tot.data(), (size_t)R));
            for (int r = 0; r < R; ++r) {
                if (!(tot[(size_t)r] <= 1.7976931348623157e308))
                    return fail(ctx, POLEE_ERR_BAD_ARG, "polee_multinomial_counts: the shares of row %d overflow", r0 + r);
                if (m > 0 && !(tot[(size_t)r] > 0.0))
                    return fail(ctx, POLEE_ERR_BAD_ARG, "polee_multinomial_counts: the shares of row %d sum to 0 with m > 0", r0 + r);
            }
            POLEE_TRY(mn_split_device(ctx, w, R, n, m, seed, first_draw + (uint64_t)r0, d_cnt.p, d_flag.p + 1));
            POLEE_TRY(d_cnt.download(ctx, counts + (size_t)r0 * n, (size_t)cnt));
        }
        int flag[2] = {0, 0};
        POLEE_TRY(d_flag.download(ctx, flag, 2));
        if (flag[1])
            return fail(ctx, POLEE_ERR_NONFINITE, "polee_multinomial_counts: a binomial variate used up its %d attempts", BINOMIAL_MAX_ATTEMPTS);
        return POLEE_OK;
    });
}

polee_status polee_debug_binomial(polee_ctx *ctx, const int64_t *N, const double *p, int64_t count, uint64_t seed, int64_t *out)
{
    return ctx_entry(ctx, "polee_debug_binomial", [&]() -> polee_status {
        if (!N || !p || !out || count < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_binomial: bad argument");
        for (int64_t i = 0; i < count; ++i)
            if (N[i] < 0 || N[i] >= ((int64_t)1 << 31) || !(p[i] >= 0.0 && p[i] <= 1.0))
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_binomial: entry %lld: N outside [0, 2^31) or p outside [0, 1]", (long long)i);
        DevBuf<int64_t> d_N, d_out;
        DevBuf<double> d_p;
        DevBuf<int> d_err;
        POLEE_TRY(d_N.upload(ctx, N, (size_t)count));
        POLEE_TRY(d_p.upload(ctx, p, (size_t)count));
        POLEE_TRY(d_out.alloc(ctx, (size_t)count));
        POLEE_TRY(d_err.alloc(ctx, 1));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(d_err.p, 0, sizeof(int), ctx->stream));
        hipLaunchKernelGGL(debug_binomial_kernel, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, ctx->stream, (const int64_t *)d_N.p,
                           (const double *)d_p.p, count, seed, d_out.p, d_err.p);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_TRY(d_out.download(ctx, out, (size_t)count));
        return check_attempts(ctx, d_err, "polee_debug_binomial");
    });
}

}  // extern "C"

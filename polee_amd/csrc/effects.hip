// Isoform effect sizes of the gene-isoform regression (estimate_isoform_effect_sizes, src/regression.jl:761-945) on the device:
// polee_effects_* of include/polee_hip.h; DESIGN.md section 3.11.
//
// Per Monte-Carlo draw t the reference draws the isoform bias x_j and every factor's isoform coefficients w_ij from their Normal
// surrogates, takes the within-gene softmax of x and of x + w_i, and records e_ij = log p_alt_j - log p_j per transcript and the
// Aitchison distance of the two compositions per gene; then an order statistic, a mean and an exceedance count over the draws of
// every (factor, transcript) and (factor, gene).  Here:
//
//   * one workgroup of 4 waves owns one (gene, factor); LANES RUN OVER DRAWS, the gene's isoforms are a serial loop of every lane.
//   * phase A: lane t takes lse_g(x), lse_g(x + w_i) (online, max-subtracted) and the first two moments of w_i over the gene of its
//     draws; d_t = lse_g(x + w_i) - lse_g(x) goes to LDS (f64 [niter]), the Aitchison distance -- which is exactly the population
//     standard deviation of w_i over the gene, the lse terms cancel in the clr difference -- to an f32 LDS row.
//   * phase B: the waves share the isoforms out; for isoform j a wave RECOMPUTES w_ij of every draw from the counter-based noise,
//     e = w_ij - d_t, and keeps |e| of its draws in an LDS row of its own (f32 [niter]).  Nothing of size [F, n, niter] exists, and a
//     gene of any number of isoforms takes the same path: the LDS holds 28 bytes per draw, whatever the gene.
//   * the k-th smallest |e| of a row is EXACT and takes no sort: non-negative floats order like their bit patterns, so the answer is
//     built from the top bit down in 31 rounds, each counting "pattern < trial" with wave ballots and popcounts.
//   * sums over draws are f64 in a fixed order (lane-serial, then a DPP wave sum); no atomics anywhere: bitwise reproducible.
//   * a gene of one isoform has e = 0 and distance 0 exactly (the reference computes log(1) - log(1)); it is answered without noise.
//
// Arithmetic: x, w, the running maxima, the sums of exponentials and d are f64; the exponentials themselves are f32 (expf of a
// non-positive f32 argument), which bounds a term's relative error by one f32 ulp.  The reference exponentiates x itself and
// underflows to log 0 where a gene's x spans more than ~700; the max-subtracted form here does not (not reproduced on purpose).
//
// Noise: Philox4x32-10 under the key `seed`, counter (transcript, draw, block, 'effx'); block b holds the streams 4b .. 4b + 3,
// stream 0 is the bias x_j, stream 1 + i the coefficient w_ij.  Two Box-Muller pairs per block, as rng.hpp's philox_randn4.  A value
// depends on (seed, draw, stream, transcript) alone, so phase B's recomputation returns phase A's numbers bit for bit.
#include "common.hpp"
#include "rng.hpp"
#include "wave.hpp"

#include <cmath>

namespace polee {

constexpr int FX_BLOCK = 256;
constexpr int FX_WAVES = FX_BLOCK / 64;
constexpr int FX_MAX_DRAWS = 4096;                  // 28 bytes of LDS per draw: 112 KiB of the CU's 160
constexpr size_t FX_LDS_PER_DRAW = 8 + 4 + 4 * FX_WAVES;

struct FxArgs {
    int n, F, niter, k;
    const int *gene_start;  // [G + 1]
    const int *members;     // [n] transcripts by gene, ascending inside a gene
    const float *qw_loc, *qw_scale, *bias_loc, *bias_scale;
    const float *zx, *zw;   // supplied noise [niter][n], [niter][F][n], or null
    uint64_t seed;
    double es, aes;         // thresholds (unused without their flag)
    int do_prob, do_aprob;
    float *min_e, *mean_e, *prob;        // [F][n]
    float *a_min, *a_mean, *a_prob;      // [F][G]
    int G;
};

__device__ inline void fx_block(uint64_t seed, uint32_t j, uint32_t t, uint32_t b, uint32_t (&c)[4])
{
    c[0] = j;
    c[1] = t;
    c[2] = b;
    c[3] = 0x65666678u;  // 'effx'
    philox4x32_10(c, seed);
}
// element e (0..3) of the block's four N(0,1): the Box-Muller pair of philox_randn4 (rng.hpp philox_box_muller) that holds it
__device__ inline float fx_normal(const uint32_t (&c)[4], int e)
{
    const uint32_t a = (e & 2) ? c[2] : c[0], b = (e & 2) ? c[3] : c[1];
    float zc, zs;
    philox_box_muller(a, b, zc, zs);
    return (e & 1) ? zs : zc;
}
__device__ inline float fx_noise_w(const FxArgs &A, int i, int j, int t)
{
    if (A.zw) return A.zw[((size_t)t * A.F + i) * A.n + j];
    uint32_t c[4];
    fx_block(A.seed, (uint32_t)j, (uint32_t)t, (uint32_t)(1 + i) >> 2, c);
    return fx_normal(c, (1 + i) & 3);
}
// running log-sum-exp: (m, s) with lse = m + log s
__device__ inline void fx_online(double &m, double &s, double v)
{
    if (v > m) {
        s = s * (double)expf((float)(m - v)) + 1.0;
        m = v;
    } else {
        s += (double)expf((float)(v - m));
    }
}

// The k-th smallest (1-based) of the wave's row of non-negative floats, and (lane 63) the f64 sum of `part` over the wave.
// Every lane reads back only the entries it wrote (t = 64 c + lane).  All 64 lanes must be here.
__device__ inline uint32_t fx_kth_bits(const float *row, int niter, int k, int lane)
{
    const int nch = (niter + 63) >> 6;
    uint32_t res = 0;
    for (int bit = 30; bit >= 0; --bit) {
        const uint32_t trial = res | (1u << bit);
        int below = 0;
        for (int c = 0; c < nch; ++c) {
            const int t = c * 64 + lane;
            const uint32_t v = t < niter ? __float_as_uint(row[t]) : 0x7fffffffu;
            below += __popcll(__ballot(v < trial));
        }
        if (below < k) res = trial;  // (wave-uniform: the answer is the largest u with #{v < u} < k)
    }
    return res;
}

__global__ __launch_bounds__(FX_BLOCK) void effects_kernel(FxArgs A)
{
    extern __shared__ double fx_lds[];
    const int g = blockIdx.x, i = blockIdx.y;
    const int beg = A.gene_start[g], m = A.gene_start[g + 1] - beg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int niter = A.niter, n = A.n;
    if (m <= 1) {  // (the whole workgroup) log 1 - log 1 and a distance between equal compositions: exact zeros
        if (tid == 0) {
            if (m == 1) {
                const size_t o = (size_t)i * n + A.members[beg];
                A.min_e[o] = 0.0f;
                A.mean_e[o] = 0.0f;
                A.prob[o] = (A.do_prob && 0.0 > A.es) ? 1.0f : 0.0f;
            }
            const size_t og = (size_t)i * A.G + g;
            A.a_min[og] = 0.0f;
            A.a_mean[og] = 0.0f;
            A.a_prob[og] = (A.do_aprob && 0.0 > A.aes) ? 1.0f : 0.0f;
        }
        return;
    }
    double *d = fx_lds;                           // [niter]
    float *arow = (float *)(fx_lds + niter);      // [niter]
    float *row = arow + niter + (size_t)wave * niter;  // [FX_WAVES][niter], this wave's
    const float *qwl = A.qw_loc + (size_t)i * n, *qws = A.qw_scale + (size_t)i * n;
    const uint32_t bw = (uint32_t)(1 + i) >> 2;
    const int ew = (1 + i) & 3;

    // ---- phase A: per draw, the two lse over the gene and the moments of w
    for (int t = tid; t < niter; t += FX_BLOCK) {
        double mx = -INFINITY, sx = 0.0, mv = -INFINITY, sv = 0.0, s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < m; ++r) {
            const int j = A.members[beg + r];
            float zx, zw;
            if (A.zx) {
                zx = A.zx[(size_t)t * n + j];
                zw = A.zw[((size_t)t * A.F + i) * n + j];
            } else {
                uint32_t c[4];
                fx_block(A.seed, (uint32_t)j, (uint32_t)t, 0u, c);
                zx = fx_normal(c, 0);
                if (bw != 0) fx_block(A.seed, (uint32_t)j, (uint32_t)t, bw, c);
                zw = fx_normal(c, ew);
            }
            const double x = (double)zx * (double)A.bias_scale[j] + (double)A.bias_loc[j];
            const double w = (double)zw * (double)qws[j] + (double)qwl[j];
            fx_online(mx, sx, x);
            fx_online(mv, sv, x + w);
            s1 += w;
            s2 += w * w;
        }
        d[t] = (mv - mx) + log(sv / sx);
        const double mean = s1 / m;
        arow[t] = (float)sqrt(fmax(s2 / m - mean * mean, 0.0));
    }
    __syncthreads();

    // ---- phase B: the waves share the isoforms out
    const int nch = (niter + 63) >> 6;
    for (int r = wave; r < m; r += FX_WAVES) {
        const int j = A.members[beg + r];
        const double loc = (double)qwl[j], scale = (double)qws[j];
        double sum = 0.0;
        int above = 0;
        for (int c = 0; c < nch; ++c) {
            const int t = c * 64 + lane;
            const bool ok = t < niter;
            float e = 0.0f;
            if (ok) {
                const double w = (double)fx_noise_w(A, i, j, t) * scale + loc;
                e = (float)(w - d[t]);
                row[t] = fabsf(e);
                sum += (double)e;
            }
            if (A.do_prob) above += __popcll(__ballot(ok && (double)e > A.es));
        }
        const uint32_t kth = fx_kth_bits(row, niter, A.k, lane);
        sum = wave_sum_to_lane63(sum);
        if (lane == 63) {
            const size_t o = (size_t)i * n + j;
            A.min_e[o] = __uint_as_float(kth);
            A.mean_e[o] = (float)(sum / niter);
            A.prob[o] = A.do_prob ? (float)((double)above / niter) : 0.0f;
        }
    }
    // ---- the gene's Aitchison distances (the last wave has the fewest isoforms)
    if (wave == FX_WAVES - 1) {
        double sum = 0.0;
        int above = 0;
        for (int c = 0; c < nch; ++c) {
            const int t = c * 64 + lane;
            const bool ok = t < niter;
            const float a = ok ? arow[t] : 0.0f;
            sum += (double)a;
            if (A.do_aprob) above += __popcll(__ballot(ok && (double)a > A.aes));
        }
        const uint32_t kth = fx_kth_bits(arow, niter, A.k, lane);
        sum = wave_sum_to_lane63(sum);
        if (lane == 63) {
            const size_t og = (size_t)i * A.G + g;
            A.a_min[og] = __uint_as_float(kth);
            A.a_mean[og] = (float)(sum / niter);
            A.a_prob[og] = A.do_aprob ? (float)((double)above / niter) : 0.0f;
        }
    }
}

}  // namespace polee

using namespace polee;

struct polee_effects {
    polee_ctx *ctx = nullptr;
    int32_t n = 0, G = 0, F = 0;
    DevBuf<int> d_gene_start, d_members;
    DevBuf<float> d_in, d_out, d_zx, d_zw;
};

extern "C" {

polee_status polee_effects_create(polee_ctx *ctx, int32_t n, int32_t G, const int32_t *gene_of, int32_t F, polee_effects **out)
{
    return ctx_entry(ctx, "polee_effects_create", [&]() -> polee_status {
        if (!out || !gene_of || n < 1 || G < 1 || F < 1 || F > 65535)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_effects_create: bad argument (n = %d, G = %d, F = %d; 1 <= F <= 65535)", n, G, F);
        // transcripts by gene: a counting sort, ascending transcript index inside a gene
        std::vector<int> start((size_t)G + 1, 0), members((size_t)n);
        for (int32_t j = 0; j < n; ++j) {
            if (gene_of[j] < 0 || gene_of[j] >= G)
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_effects_create: gene_of[%d] = %d is outside 0 .. %d", j, gene_of[j], G - 1);
            ++start[(size_t)gene_of[j] + 1];
        }
        for (int32_t g = 0; g < G; ++g) start[(size_t)g + 1] += start[(size_t)g];
        {
            std::vector<int> fill(start.begin(), start.end() - 1);
            for (int32_t j = 0; j < n; ++j) members[(size_t)fill[(size_t)gene_of[j]]++] = j;
        }
        polee_effects *fx = new polee_effects();
        fx->ctx = ctx;
        ctx_retain(ctx);
        fx->n = n;
        fx->G = G;
        fx->F = F;
        polee_status st = fx->d_gene_start.upload(ctx, start);
        if (st == POLEE_OK) st = fx->d_members.upload(ctx, members);
        if (st == POLEE_OK) st = fx->d_in.alloc(ctx, (size_t)2 * F * n + (size_t)2 * n);
        if (st == POLEE_OK) st = fx->d_out.alloc(ctx, (size_t)3 * F * n + (size_t)3 * F * G);
        if (st != POLEE_OK) {
            polee_effects_destroy(fx);
            return st;
        }
        *out = fx;
        return POLEE_OK;
    });
}

void polee_effects_destroy(polee_effects *fx)
{
    if (!fx) return;
    polee_ctx *ctx = fx->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete fx;
    ctx_release(ctx);
}

polee_status polee_effects_run(polee_effects *fx, const float *qw_loc, const float *qw_scale, const float *qx_bias_loc,
                               const float *qx_bias_scale, int32_t niter, double target_coverage, double effect_size_or_nan,
                               double aitchison_effect_size_or_nan, uint64_t seed, const float *zx_or_null, int64_t zx_len,
                               const float *zw_or_null, int64_t zw_len, float *min_effect_sizes, float *mean_effect_sizes, float *prob_de,
                               float *aitchison_min, float *aitchison_mean, float *aitchison_prob_de, double *kernel_ms_or_null)
{
    return entry(fx, "polee_effects_run", [&](polee_ctx *ctx) -> polee_status {
        const size_t n = (size_t)fx->n, F = (size_t)fx->F, G = (size_t)fx->G;
        if (!qw_loc || !qw_scale || !qx_bias_loc || !qx_bias_scale || !min_effect_sizes || !mean_effect_sizes || !prob_de ||
            !aitchison_min || !aitchison_mean || !aitchison_prob_de)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_effects_run: null argument");
        if (niter < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_effects_run: niter = %d, must be at least 1", niter);
        if (niter > FX_MAX_DRAWS)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_effects_run: niter = %d; the kernel keeps %zu bytes of LDS per draw and is built for at most %d",
                        niter, FX_LDS_PER_DRAW, FX_MAX_DRAWS);
        if (!(target_coverage > 0.0 && target_coverage <= 1.0))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_effects_run: target_coverage = %g is outside (0, 1]", target_coverage);
        if ((zx_or_null == nullptr) != (zw_or_null == nullptr))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_effects_run: give both zx and zw, or neither");
        if (zx_or_null && (zx_len != (int64_t)niter * (int64_t)n || zw_len != (int64_t)niter * (int64_t)(F * n)))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_effects_run: noise of %lld and %lld values; zx must hold niter n = %lld, zw niter F n = %lld",
                        (long long)zx_len, (long long)zw_len, (long long)niter * (long long)n, (long long)niter * (long long)(F * n));
        // Julia's round(Int, x): half to even, the default rounding mode of nearbyint (src/regression.jl:914)
        const double kr = std::nearbyint(target_coverage * (double)niter);
        const int k = (int)std::min((double)niter, std::max(1.0, kr));

        float *in = fx->d_in.p;
        const struct {
            const float *src;
            size_t off, cnt;
        } ups[4] = {{qw_loc, 0, F * n}, {qw_scale, F * n, F * n}, {qx_bias_loc, 2 * F * n, n}, {qx_bias_scale, 2 * F * n + n, n}};
        for (const auto &u : ups)
            POLEE_HIP_TRY(ctx, hipMemcpyAsync(in + u.off, u.src, u.cnt * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (host memory is borrowed for the call only)
        if (zx_or_null) {
            POLEE_TRY(fx->d_zx.upload(ctx, zx_or_null, (size_t)zx_len));
            POLEE_TRY(fx->d_zw.upload(ctx, zw_or_null, (size_t)zw_len));
        }
        FxArgs A;
        A.n = fx->n;
        A.F = fx->F;
        A.G = fx->G;
        A.niter = niter;
        A.k = k;
        A.gene_start = fx->d_gene_start.p;
        A.members = fx->d_members.p;
        A.qw_loc = in;
        A.qw_scale = in + F * n;
        A.bias_loc = in + 2 * F * n;
        A.bias_scale = in + 2 * F * n + n;
        A.zx = zx_or_null ? fx->d_zx.p : nullptr;
        A.zw = zx_or_null ? fx->d_zw.p : nullptr;
        A.seed = seed;
        A.do_prob = !std::isnan(effect_size_or_nan);
        A.do_aprob = !std::isnan(aitchison_effect_size_or_nan);
        A.es = A.do_prob ? effect_size_or_nan : 0.0;
        A.aes = A.do_aprob ? aitchison_effect_size_or_nan : 0.0;
        float *o = fx->d_out.p;
        A.min_e = o;
        A.mean_e = o + F * n;
        A.prob = o + 2 * F * n;
        A.a_min = o + 3 * F * n;
        A.a_mean = o + 3 * F * n + F * G;
        A.a_prob = o + 3 * F * n + 2 * F * G;
        const size_t lds = FX_LDS_PER_DRAW * (size_t)niter;
        if (lds > 48 * 1024)  // (per device and kernel: set before every launch that needs it)
            POLEE_HIP_TRY(ctx, hipFuncSetAttribute((const void *)effects_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        POLEE_HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        hipLaunchKernelGGL(effects_kernel, dim3((unsigned)fx->G, (unsigned)fx->F), dim3(FX_BLOCK), lds, ctx->stream, A);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (kernel_ms_or_null) {
            float ms = 0.0f;
            POLEE_HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            *kernel_ms_or_null = (double)ms;
        }
        const struct {
            float *dst;
            size_t off, cnt;
        } downs[6] = {{min_effect_sizes, 0, F * n},          {mean_effect_sizes, F * n, F * n},          {prob_de, 2 * F * n, F * n},
                      {aitchison_min, 3 * F * n, F * G},     {aitchison_mean, 3 * F * n + F * G, F * G}, {aitchison_prob_de, 3 * F * n + 2 * F * G, F * G}};
        for (const auto &dn : downs)
            POLEE_HIP_TRY(ctx, hipMemcpyAsync(dn.dst, o + dn.off, dn.cnt * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    });
}

}  // extern "C"

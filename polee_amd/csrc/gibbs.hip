// Collapsed Gibbs sampler over fragment assignments: the exact posterior of the transcript mixture given X under a Dirichlet(1)
// prior (generate_gibbs_sample, rand_gamma, convergence_stats: src/gibbs.jl:180-319), C chains at once.  DESIGN.md §3.7.
//
// Layout (built on the device at create): fragments with one compatible transcript are assigned with certainty and become a
// constant count per transcript (base); empty fragments are dropped; the others are rows of a fragment-major CSR sorted by their
// first transcript (ties by original index), cut into tiles of rows.  Per-chain state is transcript-major [n][C]: the C lanes
// that serve one fragment read one contiguous segment of g and count into adjacent words.
//
// A sweep is two launches: gb_assign_kernel (weights, one uniform, the first entry whose running sum reaches r = u sum w,
// counted in a privatised LDS histogram over the tile's transcript window, or with global atomics when the window does not fit)
// and gb_gamma_kernel (g = Gamma(1 + base + count) by Marsaglia-Tsang with an f64 acceptance test; clears the other count
// buffer for the next sweep).  A stored sweep adds gb_store_kernel (x = (g / l) / sum, f64 sum in a fixed order).
// Randomness is Philox4x32-10 keyed by (seed, sweep, chain, ORIGINAL fragment / transcript): a chain's trajectory does not
// depend on the row order, the tile size or the number of chains, and counts are integers -- a run is bitwise reproducible.
#include <cmath>

#include "common.hpp"
#include "psell_device.hpp"
#include <rocprim/rocprim.hpp>
#include "rng.hpp"
#include "../../include/polee_hip_debug.h"

using namespace polee;

namespace {

constexpr int GB_BLOCK = 256;       // threads of the assignment kernel
constexpr int GB_PASSES = 4;        // row groups a block takes in turn: a tile = GB_PASSES * GB_BLOCK / CL rows
constexpr int GB_LDS_WORDS = 8192;  // privatised histogram: window * C <= 8192 counters (32 KiB)
constexpr int GB_STORE_BLOCK = 1024;
// Philox counter (index, chain, sweep, tag << 24 | attempt); the VI noise (rng.hpp philox_randn4) has 0x70 in the tag byte
constexpr uint32_t GB_TAG_ASSIGN = 1u << 24, GB_TAG_GAMMA = 2u << 24, GB_TAG_INIT = 3u << 24;

struct GbAssign {
    int64_t M;
    const uint32_t *rowptr, *col, *orig, *tile_lo, *tile_w;
    const float *val;
    const float *g;     // [n][C]
    uint32_t *counts;   // [n][C]
    uint32_t *z;        // debug: 1-based pick of chain rec_chain per original fragment (no counting), else null
    int32_t C, cl_log, rows_per_tile, rec_chain;
    uint64_t seed;
    uint32_t sweep;
};

__device__ inline float gb_uniform(uint64_t seed, uint32_t index, uint32_t chain, uint32_t sweep)
{
    uint32_t c[4] = {index, chain, sweep, GB_TAG_ASSIGN};
    philox4x32_10(c, seed);
    // the unclamped uniform (rng.hpp): exactly 1.0f can occur here, once in 2^24 words.  The pick below still ends at the last entry
    // then: rr = 1.0f * sum and the last cs are the same f32 sum, so rr <= cs holds (tests/test_gibbs_host.py restates it bit for bit)
    return philox_u01f_raw(c[0]);
}

// One (fragment, chain) per lane; CL = 2^cl_log lanes per fragment (lanes c >= C idle).  Compiled with -ffp-contract=off: the
// weights and the running sums are the f32 products and sums that tests/test_gibbs_host.py restates.
template <bool RECORD>
__global__ __launch_bounds__(GB_BLOCK) void gb_assign_kernel(GbAssign A)
{
    __shared__ uint32_t hist[GB_LDS_WORDS];
    const int tid = threadIdx.x;
    const uint32_t tile = blockIdx.x;
    const int C = A.C;
    const uint32_t lo = A.tile_lo[tile];
    const uint32_t W = A.tile_w[tile];
    const bool use_lds = !RECORD && (uint64_t)W * (uint64_t)C <= (uint64_t)GB_LDS_WORDS;  // (uniform over the block)
    if (use_lds) {
        for (uint32_t i = tid; i < W * (uint32_t)C; i += GB_BLOCK) hist[i] = 0u;
        __syncthreads();
    }
    const int c = tid & ((1 << A.cl_log) - 1);
    const int rows_per_pass = GB_BLOCK >> A.cl_log;
    for (int pass = 0; pass < GB_PASSES; ++pass) {
        const int64_t r = (int64_t)tile * A.rows_per_tile + pass * rows_per_pass + (tid >> A.cl_log);
        if (r >= A.M || c >= C) continue;
        const uint32_t b = A.rowptr[r], e = A.rowptr[r + 1];
        float sum = 0.0f;
        for (uint32_t k = b; k < e; ++k) sum += A.val[k] * A.g[(size_t)A.col[k] * C + c];
        const uint32_t o = A.orig[r];
        const float rr = gb_uniform(A.seed, o, (uint32_t)c, A.sweep) * sum;
        uint32_t pick = A.col[b];  // (every weight 0: the first entry, as gibbs.jl:195-203 picks it)
        float cs = 0.0f;
        for (uint32_t k = b; k < e; ++k) {
            const uint32_t j = A.col[k];
            cs += A.val[k] * A.g[(size_t)j * C + c];
            if (rr <= cs) {
                pick = j;
                break;
            }
        }
        if (RECORD) {
            if (c == A.rec_chain) A.z[o] = pick + 1u;
        } else if (use_lds) {
            atomicAdd(&hist[(pick - lo) * (uint32_t)C + (uint32_t)c], 1u);
        } else {
            atomicAdd(&A.counts[(size_t)pick * C + c], 1u);
        }
    }
    if (use_lds) {
        __syncthreads();
        uint32_t *dst = A.counts + (size_t)lo * C;
        for (uint32_t i = tid; i < W * (uint32_t)C; i += GB_BLOCK) {
            const uint32_t v = hist[i];
            if (v) atomicAdd(&dst[i], v);
        }
    }
}

// Marsaglia-Tsang (rand_gamma, gibbs.jl:245-280) for shape a >= 1, scale 1: one Philox block per attempt -- a Box-Muller normal
// from words 0 and 1, the acceptance uniform from word 2.  Shape constants and the test in f64: in f32, d (1 - v + log v)
// cancels once the counts pass ~1e5.
__device__ inline double gb_gamma(double a, uint64_t seed, uint32_t j, uint32_t chain, uint32_t sweep, uint32_t tag)
{
    const double d = a - 1.0 / 3.0;
    const double cc = 1.0 / sqrt(9.0 * d);
    for (uint32_t attempt = 0; attempt < (1u << 24); ++attempt) {
        uint32_t w[4] = {j, chain, sweep, tag | attempt};
        philox4x32_10(w, seed);
        const double u1 = philox_u01d(w[0]), u2 = philox_u01d(w[1]), u = philox_u01d(w[2]);
        const double x = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
        double v = 1.0 + cc * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double xsq = x * x;
        if (u < 1.0 - 0.0331 * xsq * xsq || log(u) < 0.5 * xsq + d * (1.0 - v + log(v))) return d * v;
    }
    return d;  // (unreachable in practice: every attempt accepts with probability > 0.95)
}

struct GbGamma {
    int64_t n;
    int32_t C;
    const uint32_t *base;    // [n] or null (initial draws)
    const uint32_t *counts;  // [n][C] this sweep's, or null (initial draws)
    uint32_t *clear;         // [n][C] the other buffer: zeroed for the next sweep, or null
    float *g;                // [n][C] out
    uint32_t *bad;           // set when a draw is not finite or negative
    uint64_t seed;
    uint32_t sweep, tag;
};

__global__ __launch_bounds__(256) void gb_gamma_kernel(GbGamma P)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n * P.C) return;
    const uint32_t j = (uint32_t)(i / P.C), c = (uint32_t)(i % P.C);
    const double a = P.counts ? 1.0 + (double)P.base[j] + (double)P.counts[i] : 1.0;
    if (P.clear) P.clear[i] = 0u;
    const float gv = (float)gb_gamma(a, P.seed, j, c, P.sweep, P.tag);
    if (!(gv >= 0.0f) || !isfinite(gv)) atomicOr(P.bad, 1u);
    P.g[i] = gv;
}

// x_j = (g_j / l_j) / sum_k (g_k / l_k) (g_j / sum g without lengths) into store[c][slot][:]: one block per chain, the f64 sum in a
// fixed order (thread-strided partial sums, then a fixed tree).
__global__ __launch_bounds__(GB_STORE_BLOCK) void gb_store_kernel(int64_t n, int32_t C, const float *g, const float *efflen, float *store,
                                                                  int32_t cap, int32_t slot)
{
    __shared__ double red[GB_STORE_BLOCK];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int64_t j = tid; j < n; j += GB_STORE_BLOCK) {
        const double v = (double)g[j * C + c];
        s += efflen ? v / (double)efflen[j] : v;
    }
    red[tid] = s;
    __syncthreads();
    for (int h = GB_STORE_BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double total = red[0];
    float *out = store + ((size_t)c * cap + slot) * (size_t)n;
    for (int64_t j = tid; j < n; j += GB_STORE_BLOCK) {
        const double v = (double)g[j * C + c];
        out[j] = (float)((efflen ? v / (double)efflen[j] : v) / total);
    }
}

// split-R-hat per transcript over draws [0, count) of every chain, convergence_stats (gibbs.jl:283-319) as written: k = count / 2,
// mid = (count + 1) / 2, halves [0, mid) and [mid, count), chain variances over 1/k, B = k / (2C - 1) sum (mean - total)^2.
__global__ __launch_bounds__(256) void gb_rhat_kernel(int64_t n, int32_t C, const float *store, int32_t cap, int32_t count, float *rhat)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int k = count / 2, mid = (count + 1) / 2;
    double means[64];
    double wsum = 0.0, msum = 0.0;
    for (int c = 0; c < C; ++c) {
        const float *s = store + (size_t)c * cap * (size_t)n + j;
        for (int h = 0; h < 2; ++h) {
            const int a = h ? mid : 0, b = h ? count : mid;
            double mean = 0.0;
            for (int t = a; t < b; ++t) mean += (double)s[(size_t)t * n];
            mean /= (double)(b - a);
            double var = 0.0;
            for (int t = a; t < b; ++t) {
                const double dv = (double)s[(size_t)t * n] - mean;
                var += dv * dv;
            }
            means[h * C + c] = mean;
            msum += mean;
            wsum += var / (double)k;
        }
    }
    const double total = msum / (2.0 * C);
    double bsum = 0.0;
    for (int q = 0; q < 2 * C; ++q) bsum += (means[q] - total) * (means[q] - total);
    const double B = ((double)k / (2.0 * C - 1.0)) * bsum;
    const double W = wsum / (2.0 * C);
    const double var = ((double)(k - 1) / k) * W + (1.0 / k) * B;
    rhat[j] = (float)sqrt(var / W);
}

// ---- builder kernels ----------------------------------------------------------------------------------------------------------
// per row: entries in range and ascending (bit 0: an entry >= n; bit 1: a row not ascending)
__global__ void gb_check_rows_kernel(int64_t m, int64_t n, const uint64_t *rowptr, const uint32_t *col, uint32_t *err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    uint32_t e = 0;
    for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        if ((int64_t)col[k] >= n) e |= 1u;
        if (k > rowptr[i] && col[k] < col[k - 1]) e |= 2u;
    }
    if (e) atomicOr(err, e);
}
// sort key per row: first transcript (several), 0xFFFFFFFE (one: counted into base now), 0xFFFFFFFF (empty); class totals
__global__ void gb_classify_kernel(int64_t m, const uint64_t *rowptr, const uint32_t *col, uint32_t *key, uint32_t *idx, uint32_t *base,
                                   unsigned long long *totals)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t b = rowptr[i], len = rowptr[i + 1] - b;
    idx[i] = (uint32_t)i;
    int cls = 0;
    if (len == 0) {
        key[i] = 0xFFFFFFFFu;
        cls = 2;
    } else if (len == 1) {
        key[i] = 0xFFFFFFFEu;
        atomicAdd(&base[col[b]], 1u);
        cls = 1;
    } else {
        key[i] = col[b];
    }
    // class totals: one atomic per wave and class (30 M atomics on three words serialise: 0.35 s at C2)
    const int leader = __ffsll((unsigned long long)__ballot(1)) - 1;
    for (int q = 0; q < 3; ++q) {
        const unsigned long long k = __popcll((unsigned long long)__ballot(cls == q));
        if ((int)__lane_id() == leader && k) atomicAdd(&totals[q], k);
    }
}
__global__ void gb_rowlen_kernel(int64_t M, const uint32_t *idx_s, const uint64_t *rowptr, uint32_t *len)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > M) return;
    len[r] = r < M ? (uint32_t)(rowptr[idx_s[r] + 1] - rowptr[idx_s[r]]) : 0u;
}
__global__ void gb_gather_rows_kernel(int64_t M, const uint32_t *idx_s, const uint64_t *rowptr, const uint32_t *col, const float *val,
                                      const uint32_t *nrowptr, uint32_t *ncol, float *nval, uint32_t *orig)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= M) return;
    const uint32_t i = idx_s[r];
    orig[r] = i;
    const uint64_t b = rowptr[i], e = rowptr[i + 1];
    uint32_t o = nrowptr[r];
    for (uint64_t k = b; k < e; ++k, ++o) {
        ncol[o] = col[k];
        nval[o] = val[k];
    }
}
__global__ void gb_singles_kernel(int64_t S, const uint32_t *idx_s, const uint64_t *rowptr, const uint32_t *col, uint32_t *sorig, uint32_t *scol)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S) return;
    const uint32_t i = idx_s[r];
    sorig[r] = i;
    scol[r] = col[rowptr[i]];
}
// transcript window of every tile: [first transcript of its first row, largest transcript of its rows]
__global__ void gb_tiles_kernel(int64_t num_tiles, int32_t rows_per_tile, int64_t M, const uint32_t *rowptr, const uint32_t *col, uint32_t *lo,
                                uint32_t *w)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= num_tiles) return;
    const int64_t r0 = t * rows_per_tile, r1 = r0 + rows_per_tile < M ? r0 + rows_per_tile : M;
    const uint32_t l = col[rowptr[r0]];
    uint32_t h = l;
    for (int64_t r = r0; r < r1; ++r) h = max(h, col[rowptr[r + 1] - 1]);
    lo[t] = l;
    w[t] = h - l + 1u;
}
// [C][n] (caller's order) <-> [n][C]
__global__ void gb_to_chain_major_kernel(int64_t n, int32_t C, const float *src, float *dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * C) return;
    const int64_t c = i / n, j = i % n;
    dst[j * C + c] = src[i];
}
__global__ void gb_counts_out_kernel(int64_t n, int32_t C, const uint32_t *counts, const uint32_t *base, uint32_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * C) return;
    const int64_t c = i / n, j = i % n;
    out[i] = counts[j * C + c] + base[j];
}
__global__ void gb_scatter_singles_kernel(int64_t S, const uint32_t *sorig, const uint32_t *scol, uint32_t *z)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < S) z[sorig[r]] = scol[r] + 1u;
}

inline unsigned grid(int64_t count, int block) { return (unsigned)((count + block - 1) / block); }

}  // namespace

struct polee_gibbs {
    polee_ctx *ctx = nullptr;
    int64_t m = 0, n = 0, nnz = 0;
    int32_t C = 0, cl_log = 0, rows_per_tile = 0;
    uint64_t seed = 0;
    int64_t M = 0, num_single = 0, num_empty = 0, num_tiles = 0;
    DevBuf<uint32_t> rowptr, col, orig, tile_lo, tile_w, single_orig, single_col, base;
    DevBuf<float> val, efflen;
    DevBuf<float> g[2];
    DevBuf<uint32_t> counts[2];
    DevBuf<uint32_t> bad;
    DevBuf<float> store;
    int32_t cap = 0, stored = 0, phase = 0, phase_stride = 0;
    uint32_t sweep = 0;  // sweeps run so far; sweep s uses counts[s & 1] and its uniforms carry s
    int gi = 0;          // g[gi] is the current state, g[gi ^ 1] the state the last sweep started from
};

namespace {

#define GB_HIP(expr) POLEE_HIP_TRY(ctx, expr)

polee_status gb_init_state(polee_gibbs *G)
{
    polee_ctx *ctx = G->ctx;
    GbGamma P{G->n, G->C, nullptr, nullptr, nullptr, G->g[G->gi].p, G->bad.p, G->seed, 0u, GB_TAG_INIT};
    hipLaunchKernelGGL(gb_gamma_kernel, dim3(grid(G->n * G->C, 256)), dim3(256), 0, ctx->stream, P);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

// the sampler's layout from X by rows (0-based CSR on the device, rows by original fragment)
polee_status gb_build(polee_ctx *ctx, const PsellDevCSR &X, const float *efflens, int32_t C, uint64_t seed, polee_gibbs **out)
{
    hipStream_t stream = ctx->stream;
    const int64_t m = X.m, n = X.n;
    uint64_t nnz = 0;
    if (m > 0) {
        GB_HIP(hipMemcpyAsync(&nnz, X.rowptr.p + m, 8, hipMemcpyDeviceToHost, stream));
        GB_HIP(hipStreamSynchronize(stream));
    }
    polee_gibbs *G = new (std::nothrow) polee_gibbs();
    if (!G) return fail(ctx, POLEE_ERR_OOM, "out of host memory");
    G->ctx = ctx;
    ctx_retain(ctx);
    G->m = m;
    G->n = n;
    G->nnz = (int64_t)nnz;
    G->C = C;
    while ((1 << G->cl_log) < C) ++G->cl_log;
    G->rows_per_tile = (GB_BLOCK >> G->cl_log) * GB_PASSES;
    G->seed = seed;
    auto bail = [&](polee_status st) {
        polee_gibbs_destroy(G);
        return st;
    };
#define GB_TRY(expr)                                  \
    do {                                              \
        polee_status s__ = (expr);                    \
        if (s__ != POLEE_OK) return bail(s__);        \
    } while (0)
#define GB_HTRY(expr)                                                                                              \
    do {                                                                                                           \
        hipError_t e__ = (expr);                                                                                   \
        if (e__ != hipSuccess)                                                                                     \
            return bail(fail(ctx, e__ == hipErrorOutOfMemory ? POLEE_ERR_OOM : POLEE_ERR_HIP, "%s failed: %s (%s:%d)", \
                             #expr, hipGetErrorString(e__), __FILE__, __LINE__));                                  \
    } while (0)
    GB_TRY(G->base.alloc(ctx, (size_t)n));
    GB_HTRY(hipMemsetAsync(G->base.p, 0, (size_t)n * 4, stream));
    for (int q = 0; q < 2; ++q) {
        GB_TRY(G->g[q].alloc(ctx, (size_t)n * C));
        GB_TRY(G->counts[q].alloc(ctx, (size_t)n * C));
        GB_HTRY(hipMemsetAsync(G->counts[q].p, 0, (size_t)n * C * 4, stream));
    }
    GB_TRY(G->bad.alloc(ctx, 1));
    GB_HTRY(hipMemsetAsync(G->bad.p, 0, 4, stream));
    if (efflens) GB_TRY(G->efflen.upload(ctx, efflens, (size_t)n));
    if (m > 0) {
        DevBuf<uint32_t> err, key, key_s, idx, idx_s;
        DevBuf<unsigned long long> totals;
        GB_TRY(err.alloc(ctx, 1));
        GB_HTRY(hipMemsetAsync(err.p, 0, 4, stream));
        hipLaunchKernelGGL(gb_check_rows_kernel, dim3(grid(m, 256)), dim3(256), 0, stream, m, n, X.rowptr.p, X.col.p, err.p);
        GB_HTRY(hipGetLastError());
        uint32_t h_err = 0;
        GB_HTRY(hipMemcpyAsync(&h_err, err.p, 4, hipMemcpyDeviceToHost, stream));
        GB_HTRY(hipStreamSynchronize(stream));
        if (h_err & 1u) return bail(fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create: a transcript index is larger than n"));
        DevBuf<uint32_t> col_sorted;
        DevBuf<float> val_sorted;
        const uint32_t *colp = X.col.p;
        const float *valp = X.val_ptr;
        if (h_err & 2u) {  // (X given fragment-major with a row out of order: the rows ascending, as the CSC input gives them)
            GB_TRY(col_sorted.alloc(ctx, (size_t)nnz + 1));
            GB_TRY(val_sorted.alloc(ctx, (size_t)nnz + 1));
            size_t bytes = 0;
            DevBuf<uint8_t> tmp;
            GB_HTRY(rocprim::segmented_radix_sort_pairs(nullptr, bytes, X.col.p, col_sorted.p, X.val_ptr, val_sorted.p, (size_t)nnz, (size_t)m,
                                                        X.rowptr.p, X.rowptr.p + 1, 0, 32, stream));
            GB_TRY(tmp.alloc(ctx, bytes + 1));
            GB_HTRY(rocprim::segmented_radix_sort_pairs(tmp.p, bytes, X.col.p, col_sorted.p, X.val_ptr, val_sorted.p, (size_t)nnz, (size_t)m,
                                                        X.rowptr.p, X.rowptr.p + 1, 0, 32, stream));
            GB_HTRY(hipStreamSynchronize(stream));
            colp = col_sorted.p;
            valp = val_sorted.p;
        }
        GB_TRY(key.alloc(ctx, (size_t)m));
        GB_TRY(key_s.alloc(ctx, (size_t)m));
        GB_TRY(idx.alloc(ctx, (size_t)m));
        GB_TRY(idx_s.alloc(ctx, (size_t)m));
        GB_TRY(totals.alloc(ctx, 3));
        GB_HTRY(hipMemsetAsync(totals.p, 0, 24, stream));
        hipLaunchKernelGGL(gb_classify_kernel, dim3(grid(m, 256)), dim3(256), 0, stream, m, X.rowptr.p, colp, key.p, idx.p, G->base.p,
                           totals.p);
        GB_HTRY(hipGetLastError());
        {
            size_t bytes = 0;
            DevBuf<uint8_t> tmp;
            GB_HTRY(rocprim::radix_sort_pairs(nullptr, bytes, key.p, key_s.p, idx.p, idx_s.p, (size_t)m, 0, 32, stream));
            GB_TRY(tmp.alloc(ctx, bytes + 1));
            GB_HTRY(rocprim::radix_sort_pairs(tmp.p, bytes, key.p, key_s.p, idx.p, idx_s.p, (size_t)m, 0, 32, stream));
            unsigned long long h_tot[3] = {0, 0, 0};
            GB_HTRY(hipMemcpyAsync(h_tot, totals.p, 24, hipMemcpyDeviceToHost, stream));
            GB_HTRY(hipStreamSynchronize(stream));
            G->M = (int64_t)h_tot[0];
            G->num_single = (int64_t)h_tot[1];
            G->num_empty = (int64_t)h_tot[2];
        }
        key.release();
        key_s.release();
        idx.release();
        const int64_t M = G->M, S = G->num_single;
        if (M > 0) {
            DevBuf<uint32_t> len;
            GB_TRY(len.alloc(ctx, (size_t)M + 1));
            GB_TRY(G->rowptr.alloc(ctx, (size_t)M + 1));
            hipLaunchKernelGGL(gb_rowlen_kernel, dim3(grid(M + 1, 256)), dim3(256), 0, stream, M, idx_s.p, X.rowptr.p, len.p);
            GB_HTRY(hipGetLastError());
            size_t bytes = 0;
            DevBuf<uint8_t> tmp;
            GB_HTRY(rocprim::exclusive_scan(nullptr, bytes, len.p, G->rowptr.p, 0u, (size_t)M + 1, rocprim::plus<uint32_t>(), stream));
            GB_TRY(tmp.alloc(ctx, bytes + 1));
            GB_HTRY(rocprim::exclusive_scan(tmp.p, bytes, len.p, G->rowptr.p, 0u, (size_t)M + 1, rocprim::plus<uint32_t>(), stream));
            uint32_t mnnz = 0;
            GB_HTRY(hipMemcpyAsync(&mnnz, G->rowptr.p + M, 4, hipMemcpyDeviceToHost, stream));
            GB_HTRY(hipStreamSynchronize(stream));
            GB_TRY(G->col.alloc(ctx, (size_t)mnnz));
            GB_TRY(G->val.alloc(ctx, (size_t)mnnz));
            GB_TRY(G->orig.alloc(ctx, (size_t)M));
            hipLaunchKernelGGL(gb_gather_rows_kernel, dim3(grid(M, 256)), dim3(256), 0, stream, M, idx_s.p, X.rowptr.p, colp, valp,
                               G->rowptr.p, G->col.p, G->val.p, G->orig.p);
            GB_HTRY(hipGetLastError());
            G->num_tiles = (M + G->rows_per_tile - 1) / G->rows_per_tile;
            GB_TRY(G->tile_lo.alloc(ctx, (size_t)G->num_tiles));
            GB_TRY(G->tile_w.alloc(ctx, (size_t)G->num_tiles));
            hipLaunchKernelGGL(gb_tiles_kernel, dim3(grid(G->num_tiles, 256)), dim3(256), 0, stream, G->num_tiles, G->rows_per_tile, M,
                               G->rowptr.p, G->col.p, G->tile_lo.p, G->tile_w.p);
            GB_HTRY(hipGetLastError());
        }
        if (S > 0) {
            GB_TRY(G->single_orig.alloc(ctx, (size_t)S));
            GB_TRY(G->single_col.alloc(ctx, (size_t)S));
            hipLaunchKernelGGL(gb_singles_kernel, dim3(grid(S, 256)), dim3(256), 0, stream, S, idx_s.p + M, X.rowptr.p, colp, G->single_orig.p,
                               G->single_col.p);
            GB_HTRY(hipGetLastError());
        }
        GB_HTRY(hipStreamSynchronize(stream));
    }
    GB_TRY(gb_init_state(G));
    GB_HTRY(hipStreamSynchronize(stream));
#undef GB_TRY
#undef GB_HTRY
    *out = G;
    return POLEE_OK;
}

polee_status gb_check_create_args(polee_ctx *ctx, int64_t m, int64_t n, const float *efflens, int32_t C, polee_gibbs **out)
{
    if (!out || m < 0 || n < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create: bad argument");
    if (C < 1 || C > 32) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create: num_chains must be in 1..32 (got %d)", (int)C);
    if (n >= ((int64_t)1 << 32) - 1 || m >= ((int64_t)1 << 32) - 1)
        return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_gibbs_create: fragments and transcripts are numbered in 32 bits");
    if (efflens)
        for (int64_t j = 0; j < n; ++j)
            if (!(efflens[j] > 0.0f) || !std::isfinite(efflens[j]))
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create: effective length %lld is %g (must be finite and > 0)", (long long)j,
                            (double)efflens[j]);
    return POLEE_OK;
}

}  // namespace

extern "C" {

polee_status polee_gibbs_create(polee_ctx *ctx, int64_t m, int64_t n, const void *colptr, int colptr_bytes, const uint32_t *rowval,
                                const float *nzval, const float *efflens, int32_t num_chains, uint64_t seed, polee_gibbs **out)
{
    return ctx_entry(ctx, "polee_gibbs_create", [&]() -> polee_status {
        if (!colptr) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create: bad argument");
        POLEE_TRY(gb_check_create_args(ctx, m, n, efflens, num_chains, out));
        PsellDevCSR X;
        bool needs_host = false;
        POLEE_TRY(psell_device_rows_from_csc(ctx, m, n, colptr, colptr_bytes, rowval, nzval, nullptr, X, needs_host));
        if (needs_host) return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_gibbs_create: more than 2^32 - 2 non-zeros");
        return gb_build(ctx, X, efflens, num_chains, seed, out);
    });
}

polee_status polee_gibbs_create_from_xt(polee_ctx *ctx, int64_t m, int64_t n, const uint64_t *tcolptr, const uint32_t *trowval,
                                        const float *tnzval, const float *efflens, int32_t num_chains, uint64_t seed, polee_gibbs **out)
{
    return ctx_entry(ctx, "polee_gibbs_create_from_xt", [&]() -> polee_status {
        if (!tcolptr) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create_from_xt: bad argument");
        POLEE_TRY(gb_check_create_args(ctx, m, n, efflens, num_chains, out));
        if (tcolptr[0] != 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create_from_xt: tcolptr[0] must be 1 (1-based)");
        for (int64_t i = 0; i < m; ++i)
            if (tcolptr[i + 1] < tcolptr[i]) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create_from_xt: tcolptr is not monotone");
        if (tcolptr[m] - 1 >= (1ull << 32) - 1) return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_gibbs_create_from_xt: more than 2^32 - 2 non-zeros");
        if (tcolptr[m] > 1 && (!trowval || !tnzval)) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_create_from_xt: bad argument");
        PsellDevCSR X;
        POLEE_TRY(psell_device_rows_from_xt(ctx, m, n, tcolptr, trowval, tnzval, nullptr, false, X));
        return gb_build(ctx, X, efflens, num_chains, seed, out);
    });
}

void polee_gibbs_destroy(polee_gibbs *G)
{
    if (!G) return;
    polee_ctx *ctx = G->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete G;
    ctx_release(ctx);
}

polee_status polee_gibbs_set_state(polee_gibbs *G, const float *g0)
{
    return entry(G, "polee_gibbs_set_state", [&](polee_ctx *ctx) -> polee_status {
        if (!g0) {
            POLEE_TRY(gb_init_state(G));
            GB_HIP(hipStreamSynchronize(ctx->stream));
            return POLEE_OK;
        }
        const size_t count = (size_t)G->n * G->C;
        for (size_t i = 0; i < count; ++i)
            if (!(g0[i] >= 0.0f) || !std::isfinite(g0[i]))
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_set_state: entry %zu is %g (must be finite and >= 0)", i, (double)g0[i]);
        DevBuf<float> tmp;
        POLEE_TRY(tmp.upload(ctx, g0, count));
        hipLaunchKernelGGL(gb_to_chain_major_kernel, dim3(grid((int64_t)count, 256)), dim3(256), 0, ctx->stream, G->n, G->C, tmp.p,
                           G->g[G->gi].p);
        POLEE_KERNEL_CHECK(ctx);
        GB_HIP(hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    });
}

polee_status polee_gibbs_reserve(polee_gibbs *G, int32_t draws_per_chain)
{
    return entry(G, "polee_gibbs_reserve", [&](polee_ctx *ctx) -> polee_status {
        if (draws_per_chain < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_reserve: draws_per_chain < 0");
        GB_HIP(hipStreamSynchronize(ctx->stream));
        G->store.release();
        G->cap = 0;
        G->stored = 0;
        G->phase = 0;
        if (draws_per_chain > 0) POLEE_TRY(G->store.alloc(ctx, (size_t)G->C * draws_per_chain * (size_t)G->n));
        G->cap = draws_per_chain;
        return POLEE_OK;
    });
}

polee_status polee_gibbs_run(polee_gibbs *G, int32_t nsweeps, int32_t stride)
{
    return entry(G, "polee_gibbs_run", [&](polee_ctx *ctx) -> polee_status {
        if (nsweeps < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_run: nsweeps < 0");
        if (stride < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_run: stride < 0 (0 = burn-in, nothing stored)");
        if (stride == 0 || stride != G->phase_stride) G->phase = 0;
        G->phase_stride = stride;
        if (stride > 0) {
            if (G->cap == 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_run: no store reserved (polee_gibbs_reserve)");
            const int64_t more = ((int64_t)G->phase + nsweeps) / stride;
            if (G->stored + more > G->cap)
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_run: %lld more draws do not fit the store (%d of %d used)", (long long)more,
                            (int)G->stored, (int)G->cap);
        }
        hipStream_t stream = ctx->stream;
        const int64_t nC = G->n * G->C;
        for (int32_t s = 0; s < nsweeps; ++s) {
            const uint32_t sw = ++G->sweep;
            uint32_t *cnt = G->counts[sw & 1u].p;
            if (G->M > 0) {
                GbAssign A{G->M, G->rowptr.p, G->col.p, G->orig.p, G->tile_lo.p, G->tile_w.p, G->val.p, G->g[G->gi].p, cnt, nullptr,
                           G->C, G->cl_log, G->rows_per_tile, 0, G->seed, sw};
                hipLaunchKernelGGL(gb_assign_kernel<false>, dim3((unsigned)G->num_tiles), dim3(GB_BLOCK), 0, stream, A);
                POLEE_KERNEL_CHECK(ctx);
            }
            GbGamma P{G->n, G->C, G->base.p, cnt, G->counts[(sw + 1u) & 1u].p, G->g[G->gi ^ 1].p, G->bad.p, G->seed, sw, GB_TAG_GAMMA};
            hipLaunchKernelGGL(gb_gamma_kernel, dim3(grid(nC, 256)), dim3(256), 0, stream, P);
            POLEE_KERNEL_CHECK(ctx);
            G->gi ^= 1;
            if (stride > 0 && ++G->phase == stride) {
                hipLaunchKernelGGL(gb_store_kernel, dim3((unsigned)G->C), dim3(GB_STORE_BLOCK), 0, stream, G->n, G->C, G->g[G->gi].p,
                                   G->efflen.p, G->store.p, G->cap, G->stored);
                POLEE_KERNEL_CHECK(ctx);
                ++G->stored;
                G->phase = 0;
            }
        }
        return POLEE_OK;
    });
}

polee_status polee_gibbs_sync(polee_gibbs *G)
{
    return entry(G, "polee_gibbs_sync", [&](polee_ctx *ctx) -> polee_status {
        uint32_t bad = 0;
        GB_HIP(hipMemcpyAsync(&bad, G->bad.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        GB_HIP(hipStreamSynchronize(ctx->stream));
        if (bad) return fail(ctx, POLEE_ERR_NONFINITE, "polee_gibbs: a mixture draw was not finite");
        return POLEE_OK;
    });
}

polee_status polee_gibbs_num_stored(const polee_gibbs *G, int32_t *draws_per_chain)
{
    return entry(G, "polee_gibbs_num_stored", [&](polee_ctx *ctx) -> polee_status {
        if (!draws_per_chain) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_num_stored: null argument");
        *draws_per_chain = G->stored;
        return POLEE_OK;
    });
}

polee_status polee_gibbs_get_draws(polee_gibbs *G, int32_t first, int32_t count, float *out)
{
    return entry(G, "polee_gibbs_get_draws", [&](polee_ctx *ctx) -> polee_status {
        if (first < 0 || count < 0 || first + count > G->stored || (count > 0 && !out))
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_get_draws: draws [%d, %d) outside the %d stored", (int)first, (int)(first + count),
                        (int)G->stored);
        POLEE_TRY(polee_gibbs_sync(G));
        if (count == 0) return POLEE_OK;
        const size_t row = (size_t)count * G->n * sizeof(float);
        GB_HIP(hipMemcpy2DAsync(out, row, G->store.p + (size_t)first * G->n, (size_t)G->cap * G->n * sizeof(float), row, (size_t)G->C,
                                hipMemcpyDeviceToHost, ctx->stream));
        GB_HIP(hipStreamSynchronize(ctx->stream));
        return POLEE_OK;
    });
}

polee_status polee_gibbs_get_counts(polee_gibbs *G, uint32_t *counts)
{
    return entry(G, "polee_gibbs_get_counts", [&](polee_ctx *ctx) -> polee_status {
        if (!counts) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_get_counts: null argument");
        const int64_t nC = G->n * G->C;
        DevBuf<uint32_t> tmp;
        POLEE_TRY(tmp.alloc(ctx, (size_t)nC));
        hipLaunchKernelGGL(gb_counts_out_kernel, dim3(grid(nC, 256)), dim3(256), 0, ctx->stream, G->n, G->C, G->counts[G->sweep & 1u].p,
                           G->base.p, tmp.p);
        POLEE_KERNEL_CHECK(ctx);
        return tmp.download(ctx, counts, (size_t)nC);
    });
}

polee_status polee_gibbs_rhat(polee_gibbs *G, float *rhat)
{
    return entry(G, "polee_gibbs_rhat", [&](polee_ctx *ctx) -> polee_status {
        if (!rhat) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_rhat: null argument");
        if (G->stored < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_rhat: no stored draws");
        DevBuf<float> tmp;
        POLEE_TRY(tmp.alloc(ctx, (size_t)G->n));
        hipLaunchKernelGGL(gb_rhat_kernel, dim3(grid(G->n, 256)), dim3(256), 0, ctx->stream, G->n, G->C, G->store.p, G->cap, G->stored, tmp.p);
        POLEE_KERNEL_CHECK(ctx);
        return tmp.download(ctx, rhat, (size_t)G->n);
    });
}

polee_status polee_gibbs_get_info(const polee_gibbs *G, polee_gibbs_info *info)
{
    return entry(G, "polee_gibbs_get_info", [&](polee_ctx *ctx) -> polee_status {
        if (!info) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_gibbs_get_info: null argument");
        info->m = G->m;
        info->n = G->n;
        info->nnz = G->nnz;
        info->num_chains = G->C;
        info->num_multi_rows = G->M;
        info->num_single_rows = G->num_single;
        info->num_empty_rows = G->num_empty;
        info->multi_nnz = G->M > 0 ? (int64_t)G->col.n : 0;
        info->num_tiles = G->num_tiles;
        info->rows_per_tile = G->rows_per_tile;
        info->sweeps_done = (int64_t)G->sweep;
        return POLEE_OK;
    });
}

polee_status polee_debug_gibbs_assignments(polee_gibbs *G, int32_t chain, int32_t *z)
{
    return entry(G, "polee_debug_gibbs_assignments", [&](polee_ctx *ctx) -> polee_status {
        if (!z) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_gibbs_assignments: null argument");
        if (chain < 0 || chain >= G->C) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_gibbs_assignments: chain out of range");
        if (G->sweep == 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_debug_gibbs_assignments: no sweep has run");
        DevBuf<uint32_t> dz;
        POLEE_TRY(dz.alloc(ctx, (size_t)G->m + 1));
        GB_HIP(hipMemsetAsync(dz.p, 0, ((size_t)G->m + 1) * 4, ctx->stream));
        if (G->num_single > 0) {
            hipLaunchKernelGGL(gb_scatter_singles_kernel, dim3(grid(G->num_single, 256)), dim3(256), 0, ctx->stream, G->num_single,
                               G->single_orig.p, G->single_col.p, dz.p);
            POLEE_KERNEL_CHECK(ctx);
        }
        if (G->M > 0) {
            // the last sweep's picks again: the same kernel on the state that sweep started from, recording instead of counting
            GbAssign A{G->M, G->rowptr.p, G->col.p, G->orig.p, G->tile_lo.p, G->tile_w.p, G->val.p, G->g[G->gi ^ 1].p, nullptr, dz.p,
                       G->C, G->cl_log, G->rows_per_tile, chain, G->seed, G->sweep};
            hipLaunchKernelGGL(gb_assign_kernel<true>, dim3((unsigned)G->num_tiles), dim3(GB_BLOCK), 0, ctx->stream, A);
            POLEE_KERNEL_CHECK(ctx);
        }
        return dz.download(ctx, reinterpret_cast<uint32_t *>(z), (size_t)G->m);
    });
}

}  // extern "C"

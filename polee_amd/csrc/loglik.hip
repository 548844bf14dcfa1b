// Sparse fragment x transcript log-likelihood and gradient on gfx950.
// Replaces pAt_mul_B!/pAt_mulinv_B! (src/sparse.jl:6-40) and log_likelihood /
// factored_log_likelihood (src/likelihood.jl:36-85) with ONE pass over X that evaluates
// K expression vectors at once:
//     s_i[k] = sum_j X_ij x_j[k]
//     lp[k] += ks_i log s_i[k]
//     g_j[k] += X_ij ks_i / s_i[k]      (accumulated per tile in LDS, flushed once)
// The reference makes two passes (CSR for s, CSC for g) per draw, i.e. 2*K passes per VI
// step; this file makes one: loglik_stream_kernel (loglik_stream.hpp), a persistent launch that streams the
// uniform slices of the PSELL layout (loglik_internal.hpp) through LDS rings.
// Roofline: HBM-bound by bytes (0.25 flop/B); the two small dense products per slice run on the
// exact-f32 matrix instruction because that removes the cross-lane sums, not for flops.
// Here: the other kernels of a pass, the tile schedule and the launches; the handle is created in loglik_create.cpp.
#include "loglik_stream.hpp"

#include <algorithm>
#include <cmath>
#include <queue>

namespace polee {

// Adds q[k] of every lane into gw[c*K + k].  Lanes holding the same column id are contiguous
// (rows are pattern-sorted), so contributions are first summed per run of equal ids with a
// segmented DPP scan; only the last lane of each run touches LDS.
template <int K>
__device__ inline void scatter_runs(int c, float (&q)[K], float *gw, int lane)
{
    const int c0 = __builtin_amdgcn_readfirstlane(c);
    if (__all(c == c0)) {  // one column for the whole wavefront: plain wave sum
        float *gr = gw + c0 * K;
        wave_sum_to_lane63_n<K>(q);
        if (lane == 63) {
#pragma unroll
            for (int k = 0; k < K; ++k) atomicAdd(gr + k, q[k]);
        }
        return;
    }
    const int cprev = __builtin_amdgcn_update_dpp(-1, c, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    const unsigned long long heads = __ballot(c != cprev);  // lane 0 compares with -1: always a head
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int dist = lane - (63 - __clzll(heads & upto));  // distance to the head of this lane's run
    const int rl = lane & 15;
    const float m1 = dist >= 1 ? 1.f : 0.f, m2 = dist >= 2 ? 1.f : 0.f, m4 = dist >= 4 ? 1.f : 0.f,
                m8 = dist >= 8 ? 1.f : 0.f;
    const float mb15 = dist > rl ? 1.f : 0.f;           // run started in an earlier row of 16
    const float mb31 = dist > (lane & 31) ? 1.f : 0.f;  // run started before lane 32
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x111, 0xf>(q[k]), m1, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x112, 0xf>(q[k]), m2, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x114, 0xf>(q[k]), m4, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x118, 0xf>(q[k]), m8, q[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x142, 0xa>(q[k]), mb15, q[k]);  // row_bcast:15 -> rows 1, 3
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = fmaf(dpp_mov0<0x143, 0xc>(q[k]), mb31, q[k]);  // row_bcast:31 -> rows 2, 3
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (tail) {
        float *gr = gw + c * K;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (q[k] != 0.0f) atomicAdd(gr + k, q[k]);
    }
}

// sacc[k] += v * row[k]; rows of K floats start 8-byte aligned when K is even -> 8-byte LDS reads
template <int K>
__device__ inline void fma_row(float v, const float *row, float (&sacc)[K])
{
    if constexpr (K % 2 == 0) {
        const float2 *r2 = reinterpret_cast<const float2 *>(row);
#pragma unroll
        for (int k = 0; k < K / 2; ++k) {
            const float2 x = r2[k];
            sacc[2 * k] = fmaf(v, x.x, sacc[2 * k]);
            sacc[2 * k + 1] = fmaf(v, x.y, sacc[2 * k + 1]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) sacc[k] = fmaf(v, row[k], sacc[k]);
    }
}

// ---- stream B (and fallback for very wide rows): mixed slices ---------------------------------------
// Two sweeps over each slice straight from global memory (the second one hits L1/L2); contributions
// are summed per run of equal transcript ids with DPP before touching LDS.  Few registers -> high
// occupancy hides the latency.
template <int K, bool WANT_LP, bool HAS_KS>
__device__ inline void psell_tile_body(const PsellArgs &A, int tile, float *xw, float *gw, double *lp_red)
{
    const uint8_t *__restrict__ data = A.data;
    const uint32_t *__restrict__ slice_off = A.slice_off;
    const uint32_t *__restrict__ tile_slice = A.tile_slice;
    const uint32_t *__restrict__ tile_dict = A.tile_dict;
    const uint32_t *__restrict__ dict = A.dict;
    const float *__restrict__ slice_ks = A.slice_ks;
    const float *__restrict__ x = A.x;
    float *__restrict__ g = A.g;
    double *__restrict__ lp = A.lp;

    const uint32_t d0 = tile_dict[tile];
    const int L = (int)(tile_dict[tile + 1] - d0);
    for (int i = threadIdx.x; i < L * K; i += 256) {
        const int l = i / K, k = i - l * K;
        xw[i] = x[(size_t)dict[d0 + l] * K + k];
        gw[i] = 0.0f;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t s0 = tile_slice[tile], s1 = tile_slice[tile + 1];
    double lpacc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) lpacc[k] = 0.0;

    const int stream = psell_stream_of_tile(PsellTileBounds{A.tiles_a1, A.tiles_a1m, A.tiles_a2, A.tiles_a, A.tiles_s}, tile);
    // Deterministic mode, stream B (rows of more than 32 transcripts: rare, a fraction of a per cent of the non-zeros where they
    // occur at all): ONE wave takes all slices of the tile in order -- a wave's LDS adds retire in program order, four waves' do
    // not -- and the tile's sums are STORED to its slots of gwin, which gwin_reduce_kernel adds in tile order like every other
    // tile's; its lp goes to a slot of lpwin.  (Round 5: these tiles added with float atomics, and a sample that had any was not
    // bitwise reproducible -- one gradient entry moving by an ulp between launches on a 3 M-fragment sample with 699 such rows.)
    const bool det = A.gwin != nullptr && tile >= A.tiles_s;
    for (uint32_t s = det ? (wave == 0 ? s0 : s1) : s0 + wave; s < s1; s += det ? 1u : 4u) {
        // (the slice's format -- compact, masked or mixed -- is the reader's business: psell_slice.hpp)
        const PsellSliceReader R(data, slice_off[s], slice_off[s + 1], stream, HAS_KS, lane);
        const int w = R.w;

        // sweep 1: row sums s[k] = sum_t v[t] * x[c[t]][k]
        float sacc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) sacc[k] = 0.0f;
        int t = 0;
        for (; t + 4 <= w; t += 4) {
            float v[4];
            int c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = R.value(t + u);
                c[u] = R.col(t + u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) fma_row<K>(v[u], xw + c[u] * K, sacc);
        }
        for (; t < w; ++t) fma_row<K>(R.value(t), xw + R.col(t) * K, sacc);
        const float ksv = HAS_KS ? slice_ks[(size_t)s * 64 + lane] : 1.0f;
        float wk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            wk[k] = fast_weight(ksv, sacc[k]);
            if (WANT_LP && sacc[k] > 0.0f) lpacc[k] += (double)ksv * log((double)sacc[k]);
        }
        // sweep 2 (slice is L1/L2 resident): g[c[t]][k] += v[t] * w[k], summed per run of equal ids
        for (t = 0; t < w; ++t) {
            const float v = R.value(t);
            const int c = R.col(t);
            float q[K];
#pragma unroll
            for (int k = 0; k < K; ++k) q[k] = v * wk[k];
            scatter_runs<K>(c, q, gw, lane);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L * K; i += 256) {
        const int l = i / K, k = i - l * K;
        const float v = gw[i];
        if (det) A.gwin[(size_t)(d0 + l) * K + k] = v;
        else if (v != 0.0f) atomicAdd(g + (size_t)dict[d0 + l] * K + k, v);
    }
    if (WANT_LP) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v = lpacc[k];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
            if (lane == 0) lp_red[wave] = v;
            __syncthreads();
            if (threadIdx.x == 0) {
                const double sum = lp_red[0] + lp_red[1] + lp_red[2] + lp_red[3];
                if (det) A.lpwin[(size_t)(A.lp_slot0 + (tile - A.tiles_s)) * K + k] = sum;
                else atomicAdd(lp + k, sum);
            }
            __syncthreads();
        }
    }
}

template <int K, bool WANT_LP, bool HAS_KS>
__global__ __launch_bounds__(256) void loglik_psell_kernel(PsellArgs A, int tile_base, const uint32_t *tile_ids)
{
    extern __shared__ float lds[];
    __shared__ double lp_red[4];
    const int tile = tile_ids ? (int)tile_ids[blockIdx.x] : tile_base + (int)blockIdx.x;
    psell_tile_body<K, WANT_LP, HAS_KS>(A, tile, lds, lds + (size_t)A.lcap * K, lp_red);
}

// ---- stream C: rows kept in CSR (fragments without any structure; loglik_internal.hpp) ------------------------------------------
// Lane = fragment: row sums by gathers of x rows from global memory (x is a few MB: L2), then one float atomic per entry
// and draw.  The general fallback -- any sparsity pattern, CSR's bytes -- and slow: nothing with structure ends up here.
template <int K, bool WANT_LP, bool HAS_KS>
__global__ __launch_bounds__(256) void loglik_csr_kernel(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                        const float *__restrict__ val, const float *__restrict__ ks, int64_t rows,
                                                        const float *__restrict__ x, float *__restrict__ g, double *__restrict__ lp)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double lpacc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) lpacc[k] = 0.0;
    if (i < rows) {
        const uint32_t b = rowptr[i], e = rowptr[i + 1];
        float sacc[K];
#pragma unroll
        for (int k = 0; k < K; ++k) sacc[k] = 0.0f;
        for (uint32_t p = b; p < e; ++p) fma_row<K>(val[p], x + (size_t)col[p] * K, sacc);
        const float ksv = HAS_KS ? ks[i] : 1.0f;
        float wk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            wk[k] = fast_weight(ksv, sacc[k]);
            if (WANT_LP && sacc[k] > 0.0f) lpacc[k] = (double)ksv * log((double)sacc[k]);
        }
        for (uint32_t p = b; p < e; ++p) {
            const float v = val[p];
            float *gr = g + (size_t)col[p] * K;
#pragma unroll
            for (int k = 0; k < K; ++k) atomicAdd(gr + k, v * wk[k]);
        }
    }
    if (WANT_LP) {
        __shared__ double red[4];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v = lpacc[k];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
            __syncthreads();
            if (threadIdx.x == 0) atomicAdd(lp + k, red[0] + red[1] + red[2] + red[3]);
            __syncthreads();
        }
    }
}

// x window of every tile, contiguous: xwin[e * K + k] = x[dict[e]][k] for every dictionary entry e (tiles' dictionaries
// start at multiples of 4 entries, so a tile's window starts 16-byte aligned).  One pass over 4 B x K per entry.
template <int K>
__global__ __launch_bounds__(256) void xwin_gather_kernel(const uint32_t *__restrict__ dict, const float *__restrict__ x,
                                                         int64_t entries, float *__restrict__ xwin,
                                                         const double *__restrict__ side_part, int side_nparts,
                                                         double *__restrict__ side_out)
{
    // a thread per dictionary entry: K adjacent floats in, K adjacent floats out (8-byte accesses when K is even)
    const int64_t e = ((int64_t)blockIdx.x - (side_part ? 1 : 0)) * blockDim.x + threadIdx.x;
    if (side_part && blockIdx.x == 0) {
        // the caller's side job (polee_loglik::side_part), one workgroup in front of the gather's (it starts first): column sums of side_part in a fixed
        // order (thread t adds rows t, t + 256, ...; a wave's 64 partial sums by a fixed shuffle tree, the four waves in order) and
        // their reciprocals
        __shared__ double sm[4 * K];
        double c[K];
#pragma unroll
        for (int d = 0; d < K; ++d) c[d] = 0.0;
        for (int r = threadIdx.x; r < side_nparts; r += 256)
#pragma unroll
            for (int d = 0; d < K; ++d) c[d] += side_part[(size_t)r * K + d];
#pragma unroll
        for (int d = 0; d < K; ++d) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) c[d] += __shfl_down(c[d], o, 64);
            if ((threadIdx.x & 63) == 0) sm[(threadIdx.x >> 6) * K + d] = c[d];
        }
        __syncthreads();
        if ((int)threadIdx.x < K) {
            const double t = ((sm[threadIdx.x] + sm[K + threadIdx.x]) + sm[2 * K + threadIdx.x]) + sm[3 * K + threadIdx.x];
            side_out[threadIdx.x] = t;
            side_out[K + threadIdx.x] = 1.0 / t;
        }
        return;
    }
    if (e >= entries) return;
    const float *src = x + (size_t)dict[e] * K;
    float *dst = xwin + (size_t)e * K;
    if constexpr (K % 2 == 0) {
#pragma unroll
        for (int k = 0; k < K / 2; ++k) reinterpret_cast<float2 *>(dst)[k] = reinterpret_cast<const float2 *>(src)[k];
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) dst[k] = src[k];
    }
}

// deterministic mode, second kernel: g[j][k] += the windows' values of transcript j (tslot lists its dictionary entries,
// ascending = tile order).  A thread per (j, k) walks a short list; a transcript present in more than GWIN_HEAVY tiles
// gets a block per draw (gwin_reduce_heavy_kernel): thread t sums entries t, t + 256, ... in order and a wave's 64 partial sums are
// combined by a fixed shuffle tree -- a fixed order either way.  Block 0 also adds the workgroups' log-likelihood sums in
// workgroup order.
__global__ void gwin_reduce_kernel(const uint32_t *__restrict__ tslot_ptr, const uint32_t *__restrict__ tslot,
                                   const float *__restrict__ gwin, int K, int64_t n, float *__restrict__ g,
                                   const double *__restrict__ lpwin, int nwg, double *__restrict__ lp,
                                   const uint32_t *__restrict__ gmap)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lp && blockIdx.x == 0 && threadIdx.x < K) {
        double s = 0.0;
        for (int b = 0; b < nwg; ++b) s += lpwin[(size_t)b * K + threadIdx.x];
        lp[threadIdx.x] += s;
    }
    if (i >= n * K) return;
    const int64_t j = i / K;
    const int k = (int)(i - j * K);
    const uint32_t b = tslot_ptr[j], e1 = tslot_ptr[j + 1];
    if (e1 - b > GWIN_HEAVY) return;
    // (four entries' loads in flight at a time; the additions stay in list order)
    float s = 0.0f;
    uint32_t e = b;
    for (; e + 4 <= e1; e += 4) {
        const uint32_t t0 = tslot[e], t1 = tslot[e + 1], t2 = tslot[e + 2], t3 = tslot[e + 3];
        const float a0 = gwin[(size_t)t0 * K + k], a1 = gwin[(size_t)t1 * K + k], a2 = gwin[(size_t)t2 * K + k], a3 = gwin[(size_t)t3 * K + k];
        s = (((s + a0) + a1) + a2) + a3;
    }
    if (e + 2 <= e1) {
        const uint32_t t0 = tslot[e], t1 = tslot[e + 1];
        const float a0 = gwin[(size_t)t0 * K + k], a1 = gwin[(size_t)t1 * K + k];
        s = (s + a0) + a1;
        e += 2;
    }
    if (e < e1) s += gwin[(size_t)tslot[e] * K + k];
    g[gmap ? (size_t)gmap[j] * K + k : (size_t)i] += s;
}
// (round 5: a block of 256 threads per (heavy transcript, draw) -- it was one wave per transcript looping over the draws, 25 us per
// pass for a handful of transcripts; the order is still fixed: thread t sums entries t, t + 256, ..., a wave's 64 partial sums meet
// in a fixed shuffle tree, the four waves' sums are added in wave order)
__global__ __launch_bounds__(256) void gwin_reduce_heavy_kernel(const uint32_t *__restrict__ heavy,
                                                              const uint32_t *__restrict__ tslot_ptr,
                                                              const uint32_t *__restrict__ tslot,
                                                              const float *__restrict__ gwin, int K, float *__restrict__ g,
                                                              const uint32_t *__restrict__ gmap)
{
    __shared__ float part[4];
    const uint32_t j = heavy[blockIdx.x];
    const int k = (int)blockIdx.y;
    const uint32_t b = tslot_ptr[j], e1 = tslot_ptr[j + 1];
    float s = 0.0f;
    for (uint32_t e = b + threadIdx.x; e < e1; e += 256) s += gwin[(size_t)tslot[e] * K + k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) g[(size_t)(gmap ? gmap[j] : j) * K + k] += ((part[0] + part[1]) + part[2]) + part[3];
}

// Stream S (loglik_internal.hpp): fragments with ONE compatible transcript were collapsed at build time into cnt[j] (the
// sum of their multiplicities) and a constant; a pass adds cnt_j / x_j[k] to the gradient (the reference's
// X_ij / (X_ij x_j), sparse.jl:36 after likelihood.jl:41) and cnt_j log x_j[k] (+ the constant sum of log X_ij) to lp.
// A thread per transcript; lp: per-block partial sums, added in block order by single_lp_finish_kernel (a fixed order:
// the deterministic mode stays bitwise reproducible).
__global__ __launch_bounds__(SINGLE_THREADS) void single_rows_kernel(const float *__restrict__ cnt, const float *__restrict__ x,
                                                                    int K, int64_t n, float *__restrict__ g,
                                                                    double *__restrict__ part)
{
    __shared__ double sm[SINGLE_THREADS / 64][PSELL_MAX_K];
    const int64_t j = (int64_t)blockIdx.x * SINGLE_THREADS + threadIdx.x;
    const float c = j < n ? cnt[j] : 0.0f;
    double ls[PSELL_MAX_K];
#pragma unroll
    for (int k = 0; k < PSELL_MAX_K; ++k) ls[k] = 0.0;
    if (c != 0.0f) {
        const float *xr = x + (size_t)j * K;
        float *gr = g + (size_t)j * K;
#pragma unroll
        for (int k = 0; k < PSELL_MAX_K; ++k)
            if (k < K) {
                const float xv = xr[k];
                if (g) gr[k] += c / xv;
                if (part) ls[k] = (double)c * log((double)xv);
            }
    }
    if (!part) return;
#pragma unroll
    for (int k = 0; k < PSELL_MAX_K; ++k) {
        double v = ls[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) part[(size_t)blockIdx.x * K + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}
__global__ void single_lp_finish_kernel(const double *__restrict__ part, int nblocks, int K, double logsum, double *__restrict__ lp)
{
    const int k = threadIdx.x;
    if (k >= K) return;
    double s = logsum;
    for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * K + k];
    lp[k] += s;
}

// Cost model of the schedules, MEASURED: time of every tile of a C2 sample from a clock read per tile (diagnostic build
// POLEE_TILE_CYCLES, tools/probe/tile_cycles.py), regressed per stream on the bytes the tile streams: cycles = fixed + per KiB x
// KiB, R^2 0.6 - 0.9, mean error per tile ~15 % (round 5, profiles/r05_tile_cycles_*.txt: the wide stream on four waves):
//     A1 8.7 k + 350   A1M 9 k + 750   A2 8.7 k + 310   A2M 5 k + 1400   BN 2 k + 3100
// (dense slices cost what their bytes cost; masked ones also the matrix-core work of their union; the wide masked stream runs
// on two of the four waves; BN sweeps lane per fragment).  The first model -- bytes + 4 KiB, x 1.5 for the wide streams -- left
// the slowest workgroup 25 - 30 % above the mean.
static const double TILE_COST_FIXED[PSELL_NSTREAMS] = {8700.0, 9000.0, 8700.0, 5000.0, 2000.0, 2000.0};
static const double TILE_COST_PER_KIB[PSELL_NSTREAMS] = {350.0, 750.0, 310.0, 1400.0, 3100.0, 3100.0};
static double slices_cost(const PsellHost &h, int stream, uint32_t sa, uint32_t sb)
{
    const double kib = 0.125 * (double)((h.slice_off[sb] & PSELL_OFF_MASK) - (h.slice_off[sa] & PSELL_OFF_MASK));
    static const bool old_cost = getenv("POLEE_OLD_COST") != nullptr;  // (A/B)
    if (old_cost) return (kib * 1024.0 + 4096.0) * (stream == PSELL_A2 || stream == PSELL_A2M ? 1.5 : 1.0);
    return TILE_COST_FIXED[stream] + TILE_COST_PER_KIB[stream] * kib;
}
// The waves of a workgroup take contiguous blocks of the slices [sa, sb) of tile t with about equal matrix-core work (phase 1:
// 4 ceil(w / 4) instructions, phase 2: 8 for w <= 8, else 16 per 16 transcripts; + a fixed part): cut[0..2] = the boundaries.
// (needs the slice metadata: only while the handle is being created)
static void wave_cuts(const PsellHost &h, int64_t t, uint32_t s0, uint32_t s1, uint32_t cut[3])
{
    cut[0] = cut[1] = cut[2] = s1;
    if (t >= h.num_tiles_s) return;
    static const bool bytes_cut = getenv("POLEE_BYTES_CUT") != nullptr;  // (A/B: the waves' shares balanced on bytes)
    const int nw = h.stream_of_tile(t) != PSELL_A2M ? 4 : 2;
    // (experiment, POLEE_CUT_MODEL="a,b,c": cost = a + b x groups of four transcripts + c x (1 + groups) when the slice
    // starts a new run -- the flush of the previous set and the column lookup of the new one)
    static const char *cut_env = getenv("POLEE_CUT_MODEL");
    static double cm[3] = {0, 0, 0};
    static const bool cut_custom = cut_env && sscanf(cut_env, "%lf,%lf,%lf", &cm[0], &cm[1], &cm[2]) == 3;
    auto cost = [&](uint32_t sl) {
        const int w = h.slice_w[sl];
        if (bytes_cut) return 512.0 + 128.0 * (double)((h.slice_off[sl + 1] & PSELL_OFF_MASK) - (h.slice_off[sl] & PSELL_OFF_MASK));
        if (h.stream_of_tile(t) == PSELL_BN) return 6.0 * w + 4.0;  // (instructions per entry, not matrix-core work)
        if (cut_custom) {
            const double ng = (double)((w + 3) / 4);
            const bool cont = (h.slice_flags[sl] & 2) != 0 && sl > s0;
            return cm[0] + cm[1] * ng + (cont ? 0.0 : cm[2] * (1.0 + ng));
        }
        return 4.0 * ((w + 3) / 4) + (w <= 8 ? 8.0 : 16.0 * ((w + 15) / 16)) + 10.0;
    };
    double total = 0.0;
    for (uint32_t sl = s0; sl < s1; ++sl) total += cost(sl);
    double acc = 0.0;
    int wv = 1;
    for (uint32_t sl = s0; sl < s1 && wv < nw; ++sl) {
        acc += cost(sl);
        // a wave owns at most 63 slices (one offset per lane + the end)
        while (wv < nw && (acc >= total * wv / nw || sl + 1 - (wv == 1 ? s0 : cut[wv - 2]) >= 63u)) cut[wv++ - 1] = sl + 1;
    }
    // (the last wave takes what is left: if that is more than 63 slices -- cheap slices at the tile's start -- cut
    // by count instead; the builder keeps a tile within 63 slices per active wave)
    if (s1 - (nw > 1 ? cut[nw - 2] : s0) > 63u) {
        const uint32_t per = (s1 - s0 + (uint32_t)nw - 1) / (uint32_t)nw;
        for (int q = 1; q < nw; ++q) cut[q - 1] = std::min(s1, s0 + per * (uint32_t)q);
    }
}

void loglik_prepare_tiles(polee_loglik *ll)
{
    const PsellHost &h = ll->host;
    ll->tile_cost.assign((size_t)h.num_tiles, 0.0f);
    for (int64_t t = 0; t < h.num_tiles; ++t)
        ll->tile_cost[(size_t)t] = (float)slices_cost(h, h.stream_of_tile(t), h.tile_slice[t], h.tile_slice[t + 1]);
    ll->tile_cut.assign((size_t)3 * h.num_tiles, 0u);
    for (int64_t t = 0; t < h.num_tiles; ++t) wave_cuts(h, t, h.tile_slice[t], h.tile_slice[t + 1], &ll->tile_cut[(size_t)3 * t]);
}

// Static schedule of the streaming kernel for a grid of G workgroups: the uniform tiles sorted by cost, dealt to the
// workgroups in snake order (equal sums), and inside every workgroup's list the wide tiles (stream A2, two active
// waves) spread evenly between the A1 tiles.
polee_status loglik_ensure_schedule(polee_loglik *ll, int G)
{
    if (ll->sched_grid == G && ll->d_sched.p) return POLEE_OK;
    const PsellHost &h = ll->host;
    std::vector<uint32_t> order;
    order.reserve((size_t)h.num_tiles_s);
    for (int64_t t = 0; t < h.num_tiles_s; ++t) order.push_back((uint32_t)t);  // (the wide mixed tiles behind them go to the per-tile kernel)
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ll->tile_cost[a] > ll->tile_cost[b]; });
    // longest tile first, each to the workgroup with the least work so far (ties: the lowest index): with a handful of
    // tiles per workgroup the makespan of this greedy rule is within a few per cent of the mean load, where dealing the
    // sorted tiles out in rounds left the last round's granularity as a tail
    std::vector<std::vector<uint32_t>> lists((size_t)G);
    {
        typedef std::pair<double, int> Load;  // (work so far, workgroup)
        std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
        for (int b = 0; b < G; ++b) heap.push(Load(0.0, b));
        for (uint32_t t : order) {
            Load l = heap.top();
            heap.pop();
            lists[(size_t)l.second].push_back(t);
            l.first += (double)ll->tile_cost[t];
            heap.push(l);
        }
    }
    size_t rounds = 0;
    for (auto &l : lists) rounds = std::max(rounds, l.size());
    std::vector<PosDesc> sched((rounds + 3) * (size_t)G);  // (the kernel reads up to two rounds past a column's end)
    for (auto &d : sched) {
        d = PosDesc();
        d.tile = POS_NONE;
    }
    for (int b = 0; b < G; ++b) {
        std::vector<uint32_t> big, small;
        for (uint32_t t : lists[b]) (h.stream_of_tile(t) != PSELL_A2 && h.stream_of_tile(t) != PSELL_A2M ? big : small).push_back(t);
        const size_t n = big.size() + small.size();
        size_t ib = 0, is = 0;
        for (size_t j = 0; j < n; ++j) {
            // position j takes a small tile when the running share of small tiles falls behind (phase shifted per block)
            const size_t want = ((j + 1 + (size_t)(b % 3)) * small.size()) / (n + 2);
            const bool take_small = (is < small.size()) && (ib >= big.size() || is < want);
            const uint32_t t = take_small ? small[is++] : big[ib++];
            PosDesc &d = sched[j * (size_t)G + (size_t)b];
            d.tile = t;
            d.s0 = h.tile_slice[t];
            d.s1 = h.tile_slice[t + 1];
            d.d0 = h.tile_dict[t];
            d.L = h.tile_cols[t];
            d.c1 = ll->tile_cut[(size_t)3 * t];
            d.c2 = ll->tile_cut[(size_t)3 * t + 1];
            d.c3 = ll->tile_cut[(size_t)3 * t + 2];
        }
    }
    POLEE_TRY(ll->d_sched.upload(ll->ctx, sched));
    ll->sched_grid = G;
    if (!ll->d_sched_dyn.p) {
        // the dynamic schedule's list (any grid): the tiles by descending cost, POS_NONE behind them
        // Order: inside every stream by descending cost; the streams MERGED at equal pace (a tile's key is its rank
        // among its stream's tiles divided by their number), so that every stretch of the list holds the streams in
        // their overall proportions -- while a workgroup is on a wide tile (two of its four waves at work) its
        // neighbours on the CU are mostly on narrow ones -- and the list ends with the cheapest tiles of every stream.
        std::vector<uint32_t> dorder(order);
        {
            static const bool plain = getenv("POLEE_DYN_PLAIN_ORDER") != nullptr;  // (A/B: descending cost over all streams)
            std::vector<double> key((size_t)h.num_tiles_s, 0.0);
            size_t cnt[PSELL_NSTREAMS] = {}, seen[PSELL_NSTREAMS] = {};
            for (uint32_t t : order) ++cnt[h.stream_of_tile(t)];
            for (uint32_t t : order) {
                const int st = h.stream_of_tile(t);
                key[t] = ((double)seen[st] + 0.5) / (double)cnt[st];
                ++seen[st];
            }
            if (!plain) std::stable_sort(dorder.begin(), dorder.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
        }
        // (Round 5 tried GUIDED positions -- towards the end of the list a position was a PART of a tile, at most (work still ahead)
        // / (workgroups) cycles, so that the workgroups finish closer together: the extra positions' fixed cost outweighed the
        // better balance on every input, +0.7 .. +4 % kernel time, profiles/r05_guided_positions_ab.txt.  Whole tiles.)
        std::vector<PosDesc> plist;
        plist.reserve(dorder.size());
        for (size_t i = 0; i < dorder.size(); ++i) {
            const uint32_t t = dorder[i];
            PosDesc d = PosDesc();
            d.tile = t;
            d.s0 = h.tile_slice[t];
            d.s1 = h.tile_slice[t + 1];
            d.d0 = h.tile_dict[t];
            d.L = h.tile_cols[t];
            d.c1 = ll->tile_cut[(size_t)3 * t];
            d.c2 = ll->tile_cut[(size_t)3 * t + 1];
            d.c3 = ll->tile_cut[(size_t)3 * t + 2];
            plist.push_back(d);
        }
        ll->dyn_positions = plist.size();
        std::vector<PosDesc> dynl(plist.size() + (size_t)4 * 4 * 256 + 64);
        for (auto &d : dynl) {
            d = PosDesc();
            d.tile = POS_NONE;
        }
        std::copy(plist.begin(), plist.end(), dynl.begin());
        ll->dyn_pad = dynl.size() - plist.size();
        POLEE_TRY(ll->d_sched_dyn.upload(ll->ctx, dynl));
        std::vector<unsigned int> zero(2, 0u);
        POLEE_TRY(ll->d_dyn_ctr.upload(ll->ctx, zero));
    }
    return POLEE_OK;
}

template <int K, bool LP, bool KS, bool DET>
static polee_status launch_stream(polee_loglik *ll, PsellArgs &A, int dbg)
{
    polee_ctx *ctx = ll->ctx;
    const PsellHost &h = ll->host;
    hipStream_t st = ctx->stream;
    // a uniform slice of w transcripts occupies (w+1)*256 bytes and may start 768 bytes into a 1 KiB piece
    static_assert((PSELL_NARROW_MAX + 2) * 256 + 1024 <= STREAM_RB1, "A1 slices (+ ks row) must fit their ring");
    static_assert(psell_slice_geom(PSELL_BN, false, PSELL_MIXED_NARROW_MAX, true).bytes + 1024 <= STREAM_RB1, "BN slices (+ ks row) must fit their ring");
    static_assert((PSELL_WIDE_MAX + 3) * 256 + 1024 <= STREAM_RB2, "A2M slices (+ ks row) must fit their ring");  // (A2: wide_stream's own assertion)
    const size_t lds = stream_lds_bytes<K, DET>();
    int &occ = ll->occ_cache[K][LP ? 1 : 0][KS ? 1 : 0][DET ? 1 : 0];
    if (occ == 0) {
        int nb = 0;
        POLEE_HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, loglik_stream_kernel<K, LP, KS, DET>, 256, lds));
        occ = std::max(1, std::min(nb, 4));
        if (getenv("POLEE_DEBUG_PRINT"))
            fprintf(stderr, "[loglik] stream kernel K=%d%s: %d workgroups per CU by the occupancy query, LDS %zu B, grid %d x %d\n",
                    K, DET ? " (deterministic)" : "", nb, lds, occ, ctx->num_cus);
    }
    static const int wg_env = getenv("POLEE_STREAM_WGS_PER_CU") ? atoi(getenv("POLEE_STREAM_WGS_PER_CU")) : 0;  // (A/B)
    const int per_cu = wg_env > 0 ? std::min(wg_env, occ) : occ;
    const int G = (int)std::min<int64_t>((int64_t)per_cu * ctx->num_cus, std::max<int64_t>(h.num_tiles_s, 1));
    POLEE_TRY(loglik_ensure_schedule(ll, G));  // (built at creation for the usual grid: no host work here)
    A.sched = ll->d_sched.p;
    static const bool static_sched = getenv("POLEE_STATIC_SCHED") != nullptr;  // (A/B)
    // (The deterministic mode draws its tiles too: a tile's gradient goes to the TILE's slot of gwin, in wave order, whichever
    // workgroup works on it.  Only lp with DET keeps the static lists -- its partial sums are per workgroup.)
    static const bool det_static = getenv("POLEE_DET_STATIC") != nullptr;  // (A/B)
    if (!(DET && (LP || det_static)) && !static_sched && (size_t)3 * (size_t)G + 8 <= ll->dyn_pad) {
        A.sched_dyn = ll->d_sched_dyn.p;
        A.dyn_ctr = ll->d_dyn_ctr.p;
        // (the counter runs on from launch to launch, modulo 2^32: this launch's draws are dyn_base, dyn_base + 1, ...)
        A.dyn_base = ll->dyn_base;
        A.dyn_last = (unsigned int)(ll->dyn_positions + ll->dyn_pad - 1);
        ll->dyn_base += (uint32_t)ll->dyn_positions;
    }
    // (DET: A.gwin / A.lpwin are the caller's, and so is the reduce launch behind this one and stream B's: launch_variant)
    if (!ll->xwin_ready) {
        const bool side = ll->side_part != nullptr && !ll->side_done;
        hipLaunchKernelGGL((xwin_gather_kernel<K>), dim3((unsigned)ceil_div(ll->dict_len, 256) + (side ? 1u : 0u)), dim3(256), 0, st, A.dict,
                           A.x, ll->dict_len, ll->d_xwin.p, side ? ll->side_part : nullptr, ll->side_nparts, ll->side_out);
        if (side) ll->side_done = true;
    }
    if (ll->cur_e0) (void)hipEventRecord(ll->cur_e0, st);
    hipLaunchKernelGGL((loglik_stream_kernel<K, LP, KS, DET>), dim3((unsigned)G), dim3(256), lds, st, A, dbg);
    if (ll->cur_e1) (void)hipEventRecord(ll->cur_e1, st);
    A.lp_slot0 = G;  // (DET: stream B's tiles put their lp behind the workgroups')
    return POLEE_OK;
}

template <int K, bool LP, bool KS>
static polee_status launch_variant(polee_loglik *ll, const float *d_x, float *d_g, double *d_lp)
{
    polee_ctx *ctx = ll->ctx;
    const PsellHost &h = ll->host;
    const int lcap_all = std::max(h.max_tile_cols, 1);
    hipStream_t st = ctx->stream;
    static const bool no_ring_env = getenv("POLEE_NO_RING") != nullptr;
    const bool no_ring = no_ring_env || ll->force_mixed;
    static const int dbg = getenv("POLEE_DBG_ABLATE") ? atoi(getenv("POLEE_DBG_ABLATE")) : 0;
#ifndef POLEE_ABLATE
    static const bool dbg_told = dbg != 0 && (fprintf(stderr, "[loglik] POLEE_DBG_ABLATE is ignored by this build: the switches are compiled "
                                                              "into libpolee_hip_ablate.so only (make ablate, POLEE_HIP_LIB)\n"), true);
    (void)dbg_told;
#endif
    const LoglikRemap *rm = ll->cur_remap;
    const uint32_t *csr_col = rm && rm->csr_col ? rm->csr_col : ll->d_csr_col.p;
    PsellArgs A{ll->d_data.p, ll->d_slice_off.p, ll->d_tile_slice.p, ll->d_tile_dict.p, rm ? rm->dict : ll->d_dict.p,
                ll->d_slice_ks.p, d_x, d_g, d_lp, lcap_all, (int)h.num_tiles_a,
                (int)h.num_tiles_a1, (int)h.num_tiles_a1m, (int)h.num_tiles_a2, (int)h.num_tiles_s, ll->d_xwin.p, nullptr, nullptr, nullptr, 0u, 0u, nullptr, nullptr, 0};
    const size_t lds_psell = (size_t)2 * lcap_all * K * sizeof(float);
    // The attribute belongs to (device, kernel instance): set before every launch that needs it (a host-side table
    // write), so that a second context on another GPU of the same process gets it too; checked.
    const int64_t tiles_b = h.num_tiles - h.num_tiles_s;
    if (lds_psell > 48 * 1024 && (tiles_b > 0 || no_ring))
        POLEE_HIP_TRY(ctx, hipFuncSetAttribute((const void *)loglik_psell_kernel<K, LP, KS>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    if (!no_ring) {
        const bool det = ll->deterministic;
        if (det) {  // every tile's sums go to its slots of gwin; a transcript's slots are added in tile order afterwards
            POLEE_TRY(ll->d_gwin.alloc(ctx, (size_t)ll->dict_len * PSELL_MAX_K + 512));
            POLEE_TRY(ll->d_lpwin.alloc(ctx, ((size_t)4 * ctx->num_cus + (size_t)tiles_b) * PSELL_MAX_K));
            A.gwin = ll->d_gwin.p;
            A.lpwin = ll->d_lpwin.p;
        }
        if (h.num_tiles_s > 0) {
            if (det)
                POLEE_TRY((launch_stream<K, LP, KS, true>(ll, A, dbg)));
            else
                POLEE_TRY((launch_stream<K, LP, KS, false>(ll, A, dbg)));
        }
        if (tiles_b > 0) {
            // rows with more than 32 transcripts (rare) live in mixed tiles, which the per-tile kernel takes (float atomics; in the
            // deterministic mode one wave per tile and stores to the tile's slots, see psell_tile_body)
            hipLaunchKernelGGL((loglik_psell_kernel<K, LP, KS>), dim3((unsigned)tiles_b), dim3(256), lds_psell, st, A,
                               (int)h.num_tiles_s, (const uint32_t *)nullptr);
        }
        if (det) {
            const uint32_t *gmap = ll->cur_remap ? ll->cur_remap->index_of : nullptr;
            hipLaunchKernelGGL(gwin_reduce_kernel, dim3((unsigned)ceil_div(ll->n * K, 256)), dim3(256), 0, st, ll->d_tslot_ptr.p,
                               ll->d_tslot.p, ll->d_gwin.p, K, ll->n, A.g, LP ? ll->d_lpwin.p : nullptr, A.lp_slot0 + (int)tiles_b, A.lp, gmap);
            if (ll->d_theavy.n > 0)
                hipLaunchKernelGGL(gwin_reduce_heavy_kernel, dim3((unsigned)ll->d_theavy.n, (unsigned)K), dim3(256), 0, st, ll->d_theavy.p,
                                   ll->d_tslot_ptr.p, ll->d_tslot.p, ll->d_gwin.p, K, A.g, gmap);
        }
        if (ll->csr_rows > 0)  // stream C: rows kept in CSR (float atomics: like stream B, outside the deterministic guarantee)
            hipLaunchKernelGGL((loglik_csr_kernel<K, LP, KS>), dim3((unsigned)ceil_div(ll->csr_rows, 256)), dim3(256), 0, st,
                               ll->d_csr_rowptr.p, csr_col, ll->d_csr_val.p, ll->d_csr_ks.p, ll->csr_rows, d_x, d_g, d_lp);
    } else {
        if (ll->csr_rows > 0)
            hipLaunchKernelGGL((loglik_csr_kernel<K, LP, KS>), dim3((unsigned)ceil_div(ll->csr_rows, 256)), dim3(256), 0, st,
                               ll->d_csr_rowptr.p, csr_col, ll->d_csr_val.p, ll->d_csr_ks.p, ll->csr_rows, d_x, d_g, d_lp);
        // the cross-check switch: every tile as mixed slices with the per-run DPP kernel
        if (ll->cur_e0) (void)hipEventRecord(ll->cur_e0, st);
        hipLaunchKernelGGL((loglik_psell_kernel<K, LP, KS>), dim3((unsigned)h.num_tiles), dim3(256), lds_psell, st, A, 0,
                           (const uint32_t *)nullptr);
        if (ll->cur_e1) (void)hipEventRecord(ll->cur_e1, st);
    }
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

template <int K>
static polee_status launch_k(polee_loglik *ll, const float *d_x, float *d_g, double *d_lp)
{
    if (ll->host.num_tiles == 0 && ll->csr_rows == 0) return POLEE_OK;
    if (d_lp) return ll->has_ks ? launch_variant<K, true, true>(ll, d_x, d_g, d_lp)
                                : launch_variant<K, true, false>(ll, d_x, d_g, d_lp);
    return ll->has_ks ? launch_variant<K, false, true>(ll, d_x, d_g, d_lp)
                      : launch_variant<K, false, false>(ll, d_x, d_g, d_lp);
}

polee_status loglik_eval_device(polee_loglik *ll, const float *d_x, int K, float *d_g, double *d_lp, bool xwin_ready,
                                const LoglikRemap *remap)
{
    ll->xwin_ready = xwin_ready;
    ll->cur_remap = remap;
    polee_ctx *ctx = ll->ctx;
    if (K < 1 || K > PSELL_MAX_K) return fail(ctx, POLEE_ERR_BAD_ARG, "K must be in 1..8 (got %d)", K);
    // (the pass is a single launch: one pair of events brackets both the kernel and the pass)
    // (profiling: one pair of events brackets the dominant launch, a second pair the whole pass -- the x-window gather in
    // front of it and the mixed stream's launch behind it)
    hipEvent_t e0 = nullptr, e1 = nullptr, p0 = nullptr, p1 = nullptr;
    // (profile = N > 1: every N-th pass only.  Four event records per pass are four barrier packets in the stream -- measured
    // with rocprofv3, round 5: 22 us of idle gaps per VI iteration when EVERY pass is bracketed, 5 % of a C2 step)
    if (ll->profile && (ll->prof_every <= 1 || ll->prof_tick++ % (uint64_t)ll->prof_every == 0)) {
        if (ll->prof_used + 4 > ll->prof_events.size()) {
            if (ll->prof_events.size() >= 8192) POLEE_TRY(ll->profile_collect());
            while (ll->prof_used + 4 > ll->prof_events.size()) {
                hipEvent_t a;
                POLEE_HIP_TRY(ctx, hipEventCreate(&a));
                ll->prof_events.push_back(a);
            }
        }
        e0 = ll->prof_events[ll->prof_used];
        e1 = ll->prof_events[ll->prof_used + 1];
        p0 = ll->prof_events[ll->prof_used + 2];
        p1 = ll->prof_events[ll->prof_used + 3];
        ll->prof_used += 4;
    }
    ll->cur_e0 = e0;
    ll->cur_e1 = e1;
    if (p0) (void)hipEventRecord(p0, ctx->stream);
    polee_status st;
    switch (K) {
        case 1: st = launch_k<1>(ll, d_x, d_g, d_lp); break;
        case 2: st = launch_k<2>(ll, d_x, d_g, d_lp); break;
        case 3: st = launch_k<3>(ll, d_x, d_g, d_lp); break;
        case 4: st = launch_k<4>(ll, d_x, d_g, d_lp); break;
        case 5: st = launch_k<5>(ll, d_x, d_g, d_lp); break;
        case 6: st = launch_k<6>(ll, d_x, d_g, d_lp); break;
        case 7: st = launch_k<7>(ll, d_x, d_g, d_lp); break;
        default: st = launch_k<8>(ll, d_x, d_g, d_lp); break;
    }
    if (st != POLEE_OK && ll->d_dyn_ctr.p) {  // a failed launch may have made only some of its draws: counter and base start over
        (void)hipMemsetAsync(ll->d_dyn_ctr.p, 0, 2 * sizeof(unsigned int), ctx->stream);
        ll->dyn_base = 0;
    }
    ll->cur_remap = nullptr;
    // stream S; a caller whose forward kernel has already written cnt / x into g only needs the log-likelihood's share
    if (st == POLEE_OK && ll->has_singles && !(remap && remap->singles_in_g && !d_lp)) {
        const int nb = (int)ceil_div(ll->n, SINGLE_THREADS);
        hipLaunchKernelGGL(single_rows_kernel, dim3((unsigned)nb), dim3(SINGLE_THREADS), 0, ctx->stream,
                           remap && remap->single_cnt ? remap->single_cnt : ll->d_single_cnt.p, d_x, K,
                           ll->n, remap && remap->singles_in_g ? nullptr : d_g, d_lp ? ll->d_single_part.p : nullptr);
        if (d_lp)
            hipLaunchKernelGGL(single_lp_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, ll->d_single_part.p, nb, K,
                               ll->host.single_logsum, d_lp);
        POLEE_KERNEL_CHECK(ctx);
    }
    if (p1) (void)hipEventRecord(p1, ctx->stream);
    return st;
}

// [rows][n] <-> [n][rows] re-layout between the host API (one expression vector per row)
// and the kernel's transcript-major layout.
__global__ void rows_to_aos_kernel(const float *in, int K, int64_t n, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int64_t j = i / K;
    const int k = (int)(i - j * K);
    out[i] = in[(int64_t)k * n + j];
}
__global__ void aos_to_rows_f64_kernel(const float *in, int K, int64_t n, double *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int k = (int)(i / n);
    const int64_t j = i - (int64_t)k * n;
    out[i] = (double)in[j * K + k];
}

// effective_length_jacobian_adjustment! (src/likelihood.jl:93-110), host-pointer form.
__global__ void efflen_sum_kernel(const float *efflens, const float *xs, int64_t n, double *sums)
{
    __shared__ double smd[4];
    const int row = blockIdx.y;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s += (double)(xs[(int64_t)row * n + i] / efflens[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) smd[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[row], smd[0] + smd[1] + smd[2] + smd[3]);
}
__global__ void efflen_adjust_kernel(const float *efflens, const float *xs, const double *sums, int64_t n,
                                     double *x_grad, float *xls)
{
    const int row = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double c = sums[row];
    const float inv_l = 1.0f / efflens[i];
    x_grad[(int64_t)row * n + i] -= (double)((float)n * inv_l) / c;  // n * (1/efflens[i]) is Float32 in the reference
    if (xls) xls[(int64_t)row * n + i] = (float)((double)(xs[(int64_t)row * n + i] / efflens[i]) / c);
}

}  // namespace polee

namespace polee {
void loglik_retain(polee_loglik *ll)
{
    if (ll) ++ll->refs;
}
void loglik_release(polee_loglik *ll)
{
    if (!ll || --ll->refs > 0) return;
    polee_ctx *ctx = ll->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    for (hipEvent_t e : ll->prof_events) (void)hipEventDestroy(e);
    delete ll;
    ctx_release(ctx);
}
}  // namespace polee

using namespace polee;

polee_status polee_loglik::profile_collect()
{
    if (prof_used == 0) return POLEE_OK;
    POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i + 3 < prof_used; i += 4) {
        float ms = 0.f, pass_ms = 0.f;
        // (a sample without uniform tiles never records the kernel pair: its pass is the mixed launch)
        if (hipEventElapsedTime(&ms, prof_events[i], prof_events[i + 1]) != hipSuccess) ms = 0.f;
        POLEE_HIP_TRY(ctx, hipEventElapsedTime(&pass_ms, prof_events[i + 2], prof_events[i + 3]));
        prof_ms_total += ms;
        prof_pass_ms_total += pass_ms;
        ++prof_launches;
    }
    prof_used = 0;
    return POLEE_OK;
}

extern "C" {

polee_status polee_loglik_set_deterministic(polee_loglik *ll, int on)
{
    return entry(ll, "polee_loglik_set_deterministic", [&](polee_ctx *ctx) -> polee_status {
        ll->deterministic = on != 0;
        return POLEE_OK;
    });
}

polee_status polee_debug_loglik_force_mixed(polee_loglik *ll, int on)
{
    return entry(ll, "polee_debug_loglik_force_mixed", [&](polee_ctx *ctx) -> polee_status {
        ll->force_mixed = on != 0;
        return POLEE_OK;
    });
}

void polee_loglik_destroy(polee_loglik *ll) { loglik_release(ll); }

polee_status polee_loglik_eval(polee_loglik *ll, const float *xs, int32_t K, double *x_grad, double *lp)
{
    return entry(ll, "polee_loglik_eval", [&](polee_ctx *ctx) -> polee_status {
        if (!xs || !x_grad || K < 1 || K > PSELL_MAX_K)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_loglik_eval: bad argument (K must be 1..8)");
        const size_t n = ll->n, tot = n * K;
        POLEE_TRY(ll->d_x_rows.upload(ctx, xs, tot));
        POLEE_TRY(ll->d_x_aos.alloc(ctx, tot));
        POLEE_TRY(ll->d_g_aos.alloc(ctx, tot));
        POLEE_TRY(ll->d_g_rows.alloc(ctx, tot));
        POLEE_TRY(ll->d_lp.alloc(ctx, PSELL_MAX_K));
        const unsigned nb = (unsigned)ceil_div(tot, 256);
        hipLaunchKernelGGL(rows_to_aos_kernel, dim3(nb), dim3(256), 0, ctx->stream, ll->d_x_rows.p, K, (int64_t)n,
                           ll->d_x_aos.p);
        POLEE_HIP_TRY(ctx, hipMemsetAsync(ll->d_g_aos.p, 0, tot * sizeof(float), ctx->stream));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(ll->d_lp.p, 0, PSELL_MAX_K * sizeof(double), ctx->stream));
        POLEE_TRY(loglik_eval_device(ll, ll->d_x_aos.p, K, ll->d_g_aos.p, lp ? ll->d_lp.p : nullptr));
        hipLaunchKernelGGL(aos_to_rows_f64_kernel, dim3(nb), dim3(256), 0, ctx->stream, ll->d_g_aos.p, K, (int64_t)n,
                           ll->d_g_rows.p);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_TRY(ll->d_g_rows.download(ctx, x_grad, tot));
        if (lp) {
            POLEE_TRY(ll->d_lp.download(ctx, lp, K));
            for (int k = 0; k < K; ++k)
                if (!std::isfinite(lp[k]))
                    return fail(ctx, POLEE_ERR_NONFINITE, "log-likelihood is not finite (likelihood.jl:50)");
        }
        return POLEE_OK;
    });
}

polee_status polee_efflen_jacobian_adjustment(polee_ctx *ctx, const float *efflens, const float *xs, int32_t K,
                                              int64_t n, double *x_grad, float *xls)
{
    return ctx_entry(ctx, "polee_efflen_jacobian_adjustment", [&]() -> polee_status {
        if (!efflens || !xs || !x_grad || K < 1 || n < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_efflen_jacobian_adjustment: bad argument");
        DevBuf<float> d_l, d_x, d_xls;
        DevBuf<double> d_g, d_s;
        const size_t tot = (size_t)n * K;
        POLEE_TRY(d_l.upload(ctx, efflens, n));
        POLEE_TRY(d_x.upload(ctx, xs, tot));
        POLEE_TRY(d_g.upload(ctx, x_grad, tot));
        POLEE_TRY(d_s.alloc(ctx, K));
        if (xls) POLEE_TRY(d_xls.alloc(ctx, tot));
        POLEE_HIP_TRY(ctx, hipMemsetAsync(d_s.p, 0, K * sizeof(double), ctx->stream));
        const unsigned nb = (unsigned)std::min<int64_t>(ceil_div(n, 256), 1024);
        hipLaunchKernelGGL(efflen_sum_kernel, dim3(nb, K), dim3(256), 0, ctx->stream, d_l.p, d_x.p, n, d_s.p);
        hipLaunchKernelGGL(efflen_adjust_kernel, dim3((unsigned)ceil_div(n, 256), K), dim3(256), 0, ctx->stream, d_l.p,
                           d_x.p, d_s.p, n, d_g.p, xls ? d_xls.p : nullptr);
        POLEE_KERNEL_CHECK(ctx);
        POLEE_TRY(d_g.download(ctx, x_grad, tot));
        if (xls) POLEE_TRY(d_xls.download(ctx, xls, tot));
        return POLEE_OK;
    });
}

}  // extern "C"

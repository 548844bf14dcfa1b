// EM maximum-likelihood estimate of the transcript mixture given X (expectation_maximization, src/em.jl:3-87; `polee debug-optimize`,
// src/main.jl:960-988).  DESIGN.md §3.8.
//
// With g_j = sum_i ks_i X_ij / p_i, p_i = sum_j X_ij y_j -- the gradient a likelihood pass returns -- one EM iteration is
// y_j <- y_j g_j / M, M = sum of ks over the non-empty fragments.  The handle sits on an existing polee_loglik (no second layout of
// X) and keeps the whole loop state on the device: y, g, the pass's lp, the lp trace and a small record (EmState).  An iteration
// is polee::loglik_eval_device(ll, y, 1, g, lp) + ONE launch of em_update_kernel, which
//   * turns the pass's lp into the log-likelihood of the iterate the pass read (lp - M log sum y: y is kept to rounding, not
//     exactly, on the simplex, and at M = 3e7 a relative error of 1e-7 in sum y is 3 in lp), appends it to the trace and evaluates
//     the stop rule lp_t - lp_{t-1} < tol (em.jl:76) -- every workgroup for itself, from the same words;
//   * unless stopped, writes y <- y g / M (0 stays 0) and sums the new y in f64: per-workgroup partial sums, added in a fixed
//     order by the last workgroup to arrive (agent-scope release before its ticket, acquire behind it).  Finishing the sum in a
//     one-workgroup launch of its own was measured too and is no faster (profiles/em_bench.txt): not kept;
//   * re-zeroes g and lp for the next pass.
// Once stopped (or after a non-finite lp) y is frozen: iterations already queued leave y and the record as they are.
#include <cmath>

#include "common.hpp"
#include "loglik_internal.hpp"
#include "wave.hpp"

using namespace polee;

namespace {

constexpr int EM_BLOCK = 256;
constexpr int EM_PER_THREAD = 4;  // elements of y per thread: 1 024 per workgroup, 196 workgroups at n = 200 k
constexpr int EM_TILE = EM_BLOCK * EM_PER_THREAD;
constexpr int EM_NORM_BLOCK = 1024;
enum : int { EM_MODE_UPDATE = 0, EM_MODE_EVAL = 1 };  // EVAL: the lp of the current iterate only (the pass behind the last update)

struct EmState {
    unsigned int ticket;  // workgroups of the running launch that have delivered their partial sum (0 between launches)
    int32_t stopped;      // the stop rule fired: y is frozen
    int32_t bad;          // a non-finite lp or sum met: y is frozen, polee_em_run / _sync report POLEE_ERR_NONFINITE
    int32_t have_prev;    // prev_lp holds the lp of an iterate
    int64_t iters;        // updates made = the number of the iterate in y (0: the start)
    int64_t traced;       // trace[0 .. traced) = lp of iterates 1 .. traced
    double prev_lp;       // lp of the last iterate evaluated (of the normalised y)
    double last_inc;      // its increase over the iterate before
    double lp_start;      // lp of iterate 0
    double sum_y;         // f64 sum of y as stored
    unsigned long long kkt_bits;  // (polee_em_get_info on request) max_j y_j |g_j / M - 1| as the bits of a non-negative f64
};

struct EmArgs {
    int64_t n;
    float *y, *g;
    double *lp;       // the pass's sum of log p_i at the y it read (accumulated into: zeroed here for the next pass)
    EmState *state;
    double *partial;  // [workgroups] f64 sums of the new y
    double *trace;
    int64_t trace_cap;
    double M, tol;
    float invM;
    int32_t mode, nblocks;
};

// what this launch does, decided by every workgroup from the record the previous launch left and the pass's lp
struct EmDecision {
    bool first, record, stop, bad, update;  // first: the start's lp, nothing to compare it with
    double lp, inc;
};
__device__ inline EmDecision em_decide(const EmArgs &A)
{
    const EmState *S = A.state;
    EmDecision d{false, false, false, false, false, 0.0, 0.0};
    if (S->stopped || S->bad) return d;
    d.lp = *A.lp - A.M * log(S->sum_y);
    if (!isfinite(d.lp)) {
        d.bad = true;
        return d;
    }
    d.first = !S->have_prev;
    d.record = S->traced < S->iters;  // (false: this iterate's lp is known already -- the pass behind polee_em_run's last update)
    if (d.record && S->have_prev) {
        d.inc = d.lp - S->prev_lp;
        d.stop = A.tol >= 0.0 && d.inc < A.tol;
    }
    d.update = A.mode == EM_MODE_UPDATE && !d.stop;
    return d;
}

// by the first wave of one workgroup, all 64 lanes: the partial sums in a fixed order, then the record
__device__ inline void em_finish(const EmArgs &A, const EmDecision &d)
{
    const int lane = threadIdx.x;
    double s = 0.0;
    if (d.update)
        for (int b = lane; b < A.nblocks; b += 64) s += __hip_atomic_load(&A.partial[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s = wave_sum_to_lane63(s);
    if (lane != 63) return;
    EmState *S = A.state;
    if (d.bad) S->bad = 1;
    if (d.record) {
        if (S->traced < A.trace_cap) A.trace[S->traced] = d.lp;
        S->traced = S->iters;
        if (!d.first) S->last_inc = d.inc;
    }
    if (d.first) S->lp_start = d.lp;
    if (d.record || d.first) {
        S->prev_lp = d.lp;
        S->have_prev = 1;
    }
    if (d.stop) S->stopped = 1;
    if (d.update) {
        S->sum_y = s;
        S->iters += 1;
        if (!isfinite(s) || !(s > 0.0)) S->bad = 1;
    }
    *A.lp = 0.0;
    __hip_atomic_store(&S->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(EM_BLOCK) void em_update_kernel(EmArgs A)
{
    __shared__ double wsum[EM_BLOCK / 64];
    __shared__ int is_last;
    const int tid = threadIdx.x;
    const EmDecision d = em_decide(A);
    const int64_t base = (int64_t)blockIdx.x * EM_TILE + tid;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < EM_PER_THREAD; ++q) {
        const int64_t j = base + (int64_t)q * EM_BLOCK;
        if (j < A.n) {
            if (d.update) {
                const float yv = A.y[j];
                const float yn = yv == 0.0f ? 0.0f : yv * A.g[j] * A.invM;  // (0 stays 0 whatever g holds)
                A.y[j] = yn;
                s += (double)yn;
            }
            A.g[j] = 0.0f;
        }
    }
    s = wave_sum_to_lane63(s);
    if ((tid & 63) == 63) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        // the partial sum goes out write-through at agent scope; release, then the ticket: whoever draws the last one has every
        // workgroup's partial sum (and every workgroup's reads of the record and of lp) behind it
        __hip_atomic_store(&A.partial[blockIdx.x], ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned int t = __hip_atomic_fetch_add(&A.state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (unsigned int)A.nblocks - 1u;
        if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        is_last = last;
    }
    __syncthreads();
    if (is_last && tid < 64) em_finish(A, d);
}

// out_j = scale (y_j / l_j) / sum_k (y_k / l_k) (l = 1 without lengths): the mixture (scale 1, no lengths) and the TPMs
// (em.jl:82-84).  One workgroup, the f64 sum in a fixed order.
__global__ __launch_bounds__(EM_NORM_BLOCK) void em_normalise_kernel(int64_t n, const float *y, const float *efflen, double scale, float *out)
{
    __shared__ double red[EM_NORM_BLOCK / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t j = tid; j < n; j += EM_NORM_BLOCK) s += efflen ? (double)y[j] / (double)efflen[j] : (double)y[j];
    s = wave_sum_to_lane63(s);
    if ((tid & 63) == 63) red[tid >> 6] = s;
    __syncthreads();
    double total = 0.0;
    for (int w = 0; w < EM_NORM_BLOCK / 64; ++w) total += red[w];
    for (int64_t j = tid; j < n; j += EM_NORM_BLOCK) {
        const double v = efflen ? (double)y[j] / (double)efflen[j] : (double)y[j];
        out[j] = (float)(scale * (v / total));
    }
}

// ---- the fixed-point residual, in f64 ---------------------------------------------------------------------------------------------
// At the optimum |g_j / M - 1| is a few 1e-8, an ulp of the f32 gradient the iterations use (summed with f32 atomics: 1e-6): the
// residual takes a gradient in f64.  On request only, so simple rather than fast: the layout of X is read as it lies, slice by slice
// through PsellSliceReader (psell_slice.hpp: compact, masked and mixed slices, as loglik.hip's per-tile kernel reads them), a lane per
// fragment, row sums and weights in f64, the tile's gradient window in LDS (f64 atomics), flushed with f64 atomics; streams C and S
// likewise.  It is evaluated at the mixture polee_em_get_mixture hands out (m = the f32 of y / sum y), so that a caller can check it;
// tests/test_gpu_em.py holds this kernel against f64 NumPy on the fixture, with multiplicities, and against the f64 oracle.
struct EmG64Args {
    const uint8_t *data;
    const uint32_t *slice_off, *tile_slice, *tile_dict, *dict;
    const float *slice_ks;
    PsellTileBounds tiles;
    const float *m;  // [n]
    double *g;       // [n], zeroed
};

template <bool HAS_KS>
__global__ __launch_bounds__(256) void em_g64_tiles_kernel(EmG64Args A)
{
    __shared__ double gw[PSELL_MAX_TILE_COLS];
    const int tile = blockIdx.x;
    const uint32_t d0 = A.tile_dict[tile];
    const int L = (int)(A.tile_dict[tile + 1] - d0);
    for (int i = threadIdx.x; i < L; i += 256) gw[i] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t s0 = A.tile_slice[tile], s1 = A.tile_slice[tile + 1];
    const int stream = psell_stream_of_tile(A.tiles, tile);
    for (uint32_t s = s0 + wave; s < s1; s += 4u) {
        const PsellSliceReader R(A.data, A.slice_off[s], A.slice_off[s + 1], stream, HAS_KS, lane);
        const int w = R.w;
        double p = 0.0;
        for (int t = 0; t < w; ++t) {
            const float v = R.value(t);
            if (v != 0.0f) p += (double)v * (double)A.m[A.dict[d0 + R.col(t)]];
        }
        const double ksv = HAS_KS ? (double)A.slice_ks[(size_t)s * 64 + lane] : 1.0;
        const double wgt = p > 0.0 ? ksv / p : 0.0;  // (unused lanes: only zero values)
        if (wgt != 0.0)
            for (int t = 0; t < w; ++t) {
                const float v = R.value(t);
                if (v != 0.0f) atomicAdd(&gw[R.col(t)], (double)v * wgt);
            }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += 256)
        if (gw[i] != 0.0) atomicAdd(A.g + A.dict[d0 + i], gw[i]);
}

template <bool HAS_KS>
__global__ __launch_bounds__(256) void em_g64_csr_kernel(const uint32_t *rowptr, const uint32_t *col, const float *val, const float *ks,
                                                        int64_t rows, const float *m, double *g)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint32_t b = rowptr[i], e = rowptr[i + 1];
    double p = 0.0;
    for (uint32_t q = b; q < e; ++q) p += (double)val[q] * (double)m[col[q]];
    if (!(p > 0.0)) return;
    const double wgt = (HAS_KS ? (double)ks[i] : 1.0) / p;
    for (uint32_t q = b; q < e; ++q) atomicAdd(g + col[q], (double)val[q] * wgt);
}

// max_j (m_j / s) |g_j s / M - 1|, s = sum m, g = the sliced streams' and stream C's sum + stream S's c_j / m_j
__global__ __launch_bounds__(EM_BLOCK) void em_kkt_kernel(int64_t n, const float *m, const double *g, const float *single_cnt,
                                                          const double *msum, double M, EmState *S)
{
    const double s = *msum;
    double r = 0.0;
    for (int64_t j = (int64_t)blockIdx.x * EM_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * EM_BLOCK) {
        const double mv = (double)m[j];
        if (mv == 0.0) continue;
        double gv = g[j];
        if (single_cnt && single_cnt[j] != 0.0f) gv += (double)single_cnt[j] / mv;
        r = fmax(r, (mv / s) * fabs(gv * s / M - 1.0));
    }
    for (int o = 32; o > 0; o >>= 1) r = fmax(r, __shfl_xor(r, o, 64));
    if ((threadIdx.x & 63) == 0 && r > 0.0) atomicMax(&S->kkt_bits, (unsigned long long)__double_as_longlong(r));
}

// sum of an array of non-negative integers held as f32 (multiplicities), exact in f64 in any order
__global__ __launch_bounds__(EM_BLOCK) void em_sum_kernel(const float *a, int64_t count, double *out)
{
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * EM_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * EM_BLOCK) s += (double)a[i];
    s = wave_sum_to_lane63(s);
    if ((threadIdx.x & 63) == 63 && s != 0.0) atomicAdd(out, s);
}

inline unsigned grid(int64_t count, int block) { return (unsigned)((count + block - 1) / block); }

}  // namespace

struct polee_em {
    polee_ctx *ctx = nullptr;
    polee_loglik *ll = nullptr;
    int64_t n = 0, M = 0;
    int32_t nblocks = 0;
    DevBuf<float> y, g, out;
    DevBuf<double> lp, partial, trace;
    DevBuf<EmState> state;
    std::vector<float> single_cnt;  // stream S's counts (empty: none): a start that is 0 where one is not cannot explain its fragments
    EmState h{};                    // the record as last read
};

namespace {

#define EM_HIP(expr) POLEE_HIP_TRY(ctx, expr)

polee_status em_read_state(polee_em *E)
{
    polee_ctx *ctx = E->ctx;
    EM_HIP(hipMemcpyAsync(&E->h, E->state.p, sizeof(EmState), hipMemcpyDeviceToHost, ctx->stream));
    EM_HIP(hipStreamSynchronize(ctx->stream));
    return POLEE_OK;
}

polee_status em_nonfinite(polee_em *E)
{
    return fail(E->ctx, POLEE_ERR_NONFINITE,
                "polee_em: the log-likelihood of iterate %lld is not finite (a fragment has probability 0 under the mixture)",
                (long long)E->h.iters);
}

// M = sum of ks over the non-empty fragments
polee_status em_count_fragments(polee_em *E)
{
    polee_ctx *ctx = E->ctx;
    polee_loglik *ll = E->ll;
    if (!ll->has_ks) {
        E->M = ll->m - ll->host.empty_rows;
        return POLEE_OK;
    }
    // the multiplicities as the layout holds them: per slice lane (0 in an unused lane), per row of stream C, summed per
    // transcript in stream S
    DevBuf<double> acc;
    POLEE_TRY(acc.alloc(ctx, 1));
    EM_HIP(hipMemsetAsync(acc.p, 0, sizeof(double), ctx->stream));
    const struct {
        const float *p;
        int64_t count;
    } parts[3] = {{ll->d_slice_ks.p, std::min<int64_t>((int64_t)ll->d_slice_ks.n, ll->host.num_slices * 64)},
                  {ll->d_csr_ks.p, std::min<int64_t>((int64_t)ll->d_csr_ks.n, ll->csr_rows)},
                  {ll->has_singles ? ll->d_single_cnt.p : nullptr, ll->n}};
    for (const auto &part : parts) {
        if (!part.p || part.count <= 0) continue;
        hipLaunchKernelGGL(em_sum_kernel, dim3(std::min(grid(part.count, EM_BLOCK), 1024u)), dim3(EM_BLOCK), 0, ctx->stream, part.p,
                           part.count, acc.p);
        POLEE_KERNEL_CHECK(ctx);
    }
    double total = 0.0;
    POLEE_TRY(acc.download(ctx, &total, 1));
    E->M = (int64_t)llround(total);
    return POLEE_OK;
}

// A start with zeros must leave no fragment without a transcript.  The pass does not say so by itself: it skips a row whose sum is 0
// as it skips an unused lane, in lp and in g.  But it counts: doubling y doubles every row sum exactly (a power of two), so
// lp(2 y) - lp(y) = ln 2 x (the multiplicities of the rows it did NOT skip), and that must be M.  The difference carries the spread
// of the pass's f64 sum of lp (2e-6 at 3e7 fragments) and, with multiplicities, the f32 rounding of ks log2 s per row (1e-6 each,
// signs mixed): far from the 0.5 ln 2 that one lost fragment makes.  Two passes, only for a caller's start that has zeros; the
// handle's own state is not touched (g and lp hold nothing between runs and are left zeroed).
polee_status em_check_support(polee_em *E, const std::vector<float> &y, const char *who)
{
    polee_ctx *ctx = E->ctx;
    const size_t n = (size_t)E->n;
    std::vector<float> y2(n);
    for (size_t j = 0; j < n; ++j) y2[j] = 2.0f * y[j];
    DevBuf<float> d_y[2];
    POLEE_TRY(d_y[0].upload(ctx, y.data(), n));
    POLEE_TRY(d_y[1].upload(ctx, y2.data(), n));
    double lp[2] = {0.0, 0.0};
    for (int q = 0; q < 3; ++q) {  // (the third round only zeroes g and lp again)
        EM_HIP(hipMemsetAsync(E->g.p, 0, n * sizeof(float), ctx->stream));
        EM_HIP(hipMemsetAsync(E->lp.p, 0, sizeof(double), ctx->stream));
        if (q == 2) break;
        POLEE_TRY(loglik_eval_device(E->ll, d_y[q].p, 1, E->g.p, E->lp.p));
        POLEE_TRY(E->lp.download(ctx, &lp[q], 1));
    }
    EM_HIP(hipStreamSynchronize(ctx->stream));
    const double alive = (lp[1] - lp[0]) / 0.693147180559945309417;
    if (!(alive > (double)E->M - 0.5))
        return fail(ctx, POLEE_ERR_BAD_ARG,
                    "%s: %.0f of the %lld fragments have probability 0 under y0: it is 0 on every transcript they are compatible with",
                    who, std::isfinite(alive) ? (double)E->M - std::round(alive) : (double)E->M, (long long)E->M);
    return POLEE_OK;
}

// the start: y0 normalised (f64 on the host), or 1 / n (em.jl:22); everything else as new
polee_status em_set_start(polee_em *E, const float *y0, const char *who)
{
    polee_ctx *ctx = E->ctx;
    const int64_t n = E->n;
    std::vector<float> y((size_t)n);
    if (y0) {
        double total = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            if (!(y0[j] >= 0.0f) || !std::isfinite(y0[j]))
                return fail(ctx, POLEE_ERR_BAD_ARG, "%s: y0[%lld] is %g (must be finite and >= 0)", who, (long long)j, (double)y0[j]);
            total += (double)y0[j];
        }
        if (!(total > 0.0) || !std::isfinite(total)) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: y0 sums to %g (must be > 0)", who, total);
        for (int64_t j = 0; j < n; ++j) y[(size_t)j] = (float)((double)y0[j] / total);
        for (int64_t j = 0; j < n && !E->single_cnt.empty(); ++j)
            if (y[(size_t)j] == 0.0f && E->single_cnt[(size_t)j] > 0.0f)
                return fail(ctx, POLEE_ERR_BAD_ARG,
                            "%s: y0[%lld] is 0, but transcript %lld is the only one %g fragment(s) are compatible with: their probability "
                            "would be 0",
                            who, (long long)j, (long long)j, (double)E->single_cnt[(size_t)j]);
    } else {
        std::fill(y.begin(), y.end(), (float)(1.0 / (double)n));
    }
    EM_HIP(hipStreamSynchronize(ctx->stream));
    if (y0 && std::find(y.begin(), y.end(), 0.0f) != y.end()) POLEE_TRY(em_check_support(E, y, who));
    EmState s{};
    for (int64_t j = 0; j < n; ++j) s.sum_y += (double)y[(size_t)j];
    s.lp_start = s.prev_lp = s.last_inc = std::nan("");
    EM_HIP(hipMemcpyAsync(E->y.p, y.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    EM_HIP(hipMemsetAsync(E->g.p, 0, (size_t)n * sizeof(float), ctx->stream));
    EM_HIP(hipMemsetAsync(E->lp.p, 0, sizeof(double), ctx->stream));
    EM_HIP(hipMemcpyAsync(E->state.p, &s, sizeof(EmState), hipMemcpyHostToDevice, ctx->stream));
    EM_HIP(hipStreamSynchronize(ctx->stream));
    E->h = s;
    return POLEE_OK;
}

polee_status em_grow_trace(polee_em *E, int64_t need)
{
    polee_ctx *ctx = E->ctx;
    if ((int64_t)E->trace.n >= need) return POLEE_OK;
    DevBuf<double> bigger;
    POLEE_TRY(bigger.alloc(ctx, (size_t)std::max<int64_t>(need, 2 * (int64_t)E->trace.n)));
    if (E->h.traced > 0)
        EM_HIP(hipMemcpyAsync(bigger.p, E->trace.p, (size_t)E->h.traced * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    E->trace.take(bigger);
    return POLEE_OK;
}

// one likelihood pass at y + the update (or, EVAL, only the bookkeeping of the iterate's lp)
polee_status em_enqueue(polee_em *E, int mode, double tol)
{
    polee_ctx *ctx = E->ctx;
    POLEE_TRY(loglik_eval_device(E->ll, E->y.p, 1, E->g.p, E->lp.p));
    EmArgs A{E->n, E->y.p, E->g.p, E->lp.p, E->state.p, E->partial.p, E->trace.p, (int64_t)E->trace.n, (double)E->M, tol,
             (float)(1.0 / (double)E->M), mode, E->nblocks};
    hipLaunchKernelGGL(em_update_kernel, dim3((unsigned)E->nblocks), dim3(EM_BLOCK), 0, ctx->stream, A);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

polee_status em_normalised(polee_em *E, const float *d_efflen, double scale, float *out)
{
    polee_ctx *ctx = E->ctx;
    POLEE_TRY(E->out.alloc(ctx, (size_t)E->n));
    hipLaunchKernelGGL(em_normalise_kernel, dim3(1), dim3(EM_NORM_BLOCK), 0, ctx->stream, E->n, E->y.p, d_efflen, scale, E->out.p);
    POLEE_KERNEL_CHECK(ctx);
    return E->out.download(ctx, out, (size_t)E->n);
}

// the f64 gradient at the mixture handed out and its fixed-point residual, into the record
polee_status em_residual64(polee_em *E)
{
    polee_ctx *ctx = E->ctx;
    polee_loglik *ll = E->ll;
    const PsellHost &h = ll->host;
    hipStream_t stream = ctx->stream;
    DevBuf<double> g64, msum;
    POLEE_TRY(g64.alloc(ctx, (size_t)E->n));
    POLEE_TRY(msum.alloc(ctx, 1));
    POLEE_TRY(E->out.alloc(ctx, (size_t)E->n));
    EM_HIP(hipMemsetAsync(g64.p, 0, (size_t)E->n * sizeof(double), stream));
    EM_HIP(hipMemsetAsync(msum.p, 0, sizeof(double), stream));
    EM_HIP(hipMemsetAsync(&E->state.p->kkt_bits, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(em_normalise_kernel, dim3(1), dim3(EM_NORM_BLOCK), 0, stream, E->n, E->y.p, (const float *)nullptr, 1.0, E->out.p);
    hipLaunchKernelGGL(em_sum_kernel, dim3(std::min(grid(E->n, EM_BLOCK), 1024u)), dim3(EM_BLOCK), 0, stream, E->out.p, E->n, msum.p);
    POLEE_KERNEL_CHECK(ctx);
    if (h.num_tiles > 0) {
        // (a tile's dictionary is padded to a multiple of PSELL_DICT_ALIGN entries: that many slots of the kernel's LDS window)
        if (ceil_div(h.max_tile_cols, PSELL_DICT_ALIGN) * PSELL_DICT_ALIGN > PSELL_MAX_TILE_COLS)
            return fail(ctx, POLEE_ERR_UNSUPPORTED, "polee_em_get_info: a tile dictionary of %d entries", (int)h.max_tile_cols);
        EmG64Args A{ll->d_data.p, ll->d_slice_off.p, ll->d_tile_slice.p, ll->d_tile_dict.p, ll->d_dict.p, ll->d_slice_ks.p,
                    h.tile_bounds(), E->out.p, g64.p};
        if (ll->has_ks) hipLaunchKernelGGL(em_g64_tiles_kernel<true>, dim3((unsigned)h.num_tiles), dim3(256), 0, stream, A);
        else hipLaunchKernelGGL(em_g64_tiles_kernel<false>, dim3((unsigned)h.num_tiles), dim3(256), 0, stream, A);
        POLEE_KERNEL_CHECK(ctx);
    }
    if (ll->csr_rows > 0) {
        if (ll->has_ks)
            hipLaunchKernelGGL(em_g64_csr_kernel<true>, dim3(grid(ll->csr_rows, 256)), dim3(256), 0, stream, ll->d_csr_rowptr.p, ll->d_csr_col.p,
                               ll->d_csr_val.p, ll->d_csr_ks.p, ll->csr_rows, E->out.p, g64.p);
        else
            hipLaunchKernelGGL(em_g64_csr_kernel<false>, dim3(grid(ll->csr_rows, 256)), dim3(256), 0, stream, ll->d_csr_rowptr.p, ll->d_csr_col.p,
                               ll->d_csr_val.p, (const float *)nullptr, ll->csr_rows, E->out.p, g64.p);
        POLEE_KERNEL_CHECK(ctx);
    }
    hipLaunchKernelGGL(em_kkt_kernel, dim3(std::min(grid(E->n, EM_BLOCK), 1024u)), dim3(EM_BLOCK), 0, stream, E->n, E->out.p, g64.p,
                       ll->has_singles ? ll->d_single_cnt.p : (const float *)nullptr, msum.p, (double)E->M, E->state.p);
    POLEE_KERNEL_CHECK(ctx);
    EM_HIP(hipStreamSynchronize(stream));
    return POLEE_OK;
}

}  // namespace

extern "C" {

polee_status polee_em_create(polee_loglik *ll, const float *y0, polee_em **out)
{
    return entry(ll, "polee_em_create", [&](polee_ctx *ctx) -> polee_status {
        if (!out) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_create: null output pointer");
        polee_em *E = new (std::nothrow) polee_em();
        if (!E) return fail(ctx, POLEE_ERR_OOM, "out of host memory");
        E->ctx = ctx;
        ctx_retain(ctx);
        E->ll = ll;
        loglik_retain(ll);
        E->n = ll->n;
        E->nblocks = (int32_t)grid(E->n, EM_TILE);
        auto bail = [&](polee_status st) {
            polee_em_destroy(E);
            return st;
        };
        polee_status st;
        if ((st = E->y.alloc(ctx, (size_t)E->n)) || (st = E->g.alloc(ctx, (size_t)E->n)) || (st = E->lp.alloc(ctx, 1)) ||
            (st = E->partial.alloc(ctx, (size_t)E->nblocks)) || (st = E->state.alloc(ctx, 1)) || (st = E->trace.alloc(ctx, 1024)) ||
            (st = em_count_fragments(E)))
            return bail(st);
        if (E->M < 1) return bail(fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_create: no fragment is compatible with any transcript"));
        if (ll->has_singles) {
            E->single_cnt.resize((size_t)E->n);
            if ((st = ll->d_single_cnt.download(ctx, E->single_cnt.data(), (size_t)E->n))) return bail(st);
        }
        if ((st = em_set_start(E, y0, "polee_em_create"))) return bail(st);
        *out = E;
        return POLEE_OK;
    });
}

void polee_em_destroy(polee_em *E)
{
    if (!E) return;
    polee_ctx *ctx = E->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    polee_loglik *ll = E->ll;
    delete E;
    loglik_release(ll);
    ctx_release(ctx);
}

polee_status polee_em_reset(polee_em *E, const float *y0)
{
    return entry(E, "polee_em_reset", [&](polee_ctx *ctx) -> polee_status {
        return em_set_start(E, y0, "polee_em_reset");
    });
}

polee_status polee_em_run(polee_em *E, int32_t max_iters, double tol, int32_t check_every)
{
    return entry(E, "polee_em_run", [&](polee_ctx *ctx) -> polee_status {
        if (max_iters < 0) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_run: max_iters < 0");
        if (check_every < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_run: check_every < 1");
        if (std::isnan(tol)) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_run: tol is NaN");
        if (E->h.bad) return em_nonfinite(E);
        if (E->h.stopped) return POLEE_OK;
        POLEE_TRY(em_grow_trace(E, E->h.iters + max_iters));
        int32_t left = max_iters;
        do {
            const int32_t c = std::min(check_every, left);
            for (int32_t q = 0; q < c; ++q) POLEE_TRY(em_enqueue(E, EM_MODE_UPDATE, tol));
            left -= c;
            // the last iterate's lp needs a pass of its own: it rides behind the last chunk
            if (left == 0) POLEE_TRY(em_enqueue(E, EM_MODE_EVAL, tol));
            POLEE_TRY(em_read_state(E));
            if (E->h.bad) return em_nonfinite(E);
        } while (left > 0 && !E->h.stopped);
        return POLEE_OK;
    });
}

polee_status polee_em_sync(polee_em *E)
{
    return entry(E, "polee_em_sync", [&](polee_ctx *ctx) -> polee_status {
        POLEE_TRY(em_read_state(E));
        if (E->h.bad) return em_nonfinite(E);
        return POLEE_OK;
    });
}

polee_status polee_em_get_mixture(polee_em *E, float *y)
{
    return entry(E, "polee_em_get_mixture", [&](polee_ctx *ctx) -> polee_status {
        if (!y) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_get_mixture: null argument");
        return em_normalised(E, nullptr, 1.0, y);
    });
}

polee_status polee_em_get_tpm(polee_em *E, const float *efflens, float *tpm)
{
    return entry(E, "polee_em_get_tpm", [&](polee_ctx *ctx) -> polee_status {
        if (!tpm) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_get_tpm: null argument");
        DevBuf<float> d_l;
        if (efflens) {
            for (int64_t j = 0; j < E->n; ++j)
                if (!(efflens[j] > 0.0f) || !std::isfinite(efflens[j]))
                    return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_get_tpm: effective length %lld is %g (must be finite and > 0)", (long long)j,
                                (double)efflens[j]);
            POLEE_TRY(d_l.upload(ctx, efflens, (size_t)E->n));
        }
        return em_normalised(E, d_l.p, 1e6, tpm);
    });
}

polee_status polee_em_get_trace(polee_em *E, double *lp, int64_t capacity, int64_t *count)
{
    return entry(E, "polee_em_get_trace", [&](polee_ctx *ctx) -> polee_status {
        if (capacity < 0 || (capacity > 0 && !lp)) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_get_trace: capacity < 0 or a null buffer");
        POLEE_TRY(em_read_state(E));
        if (count) *count = E->h.traced;
        return E->trace.download(ctx, lp, (size_t)std::min<int64_t>(capacity, E->h.traced));
    });
}

polee_status polee_em_get_info(polee_em *E, int compute_kkt, polee_em_info *info)
{
    return entry(E, "polee_em_get_info", [&](polee_ctx *ctx) -> polee_status {
        if (!info) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_em_get_info: null argument");
        if (compute_kkt) POLEE_TRY(em_residual64(E));
        POLEE_TRY(em_read_state(E));
        info->n = E->n;
        info->M = E->M;
        info->iters = E->h.iters;
        info->converged = E->h.stopped;
        info->nonfinite = E->h.bad;
        info->lp_start = E->h.lp_start;
        info->last_lp = E->h.prev_lp;
        info->last_increase = E->h.last_inc;
        info->sum_y = E->h.sum_y;
        double kkt;
        memcpy(&kkt, &E->h.kkt_bits, sizeof kkt);
        info->kkt_max = compute_kkt ? kkt : -1.0;
        return POLEE_OK;
    });
}

}  // extern "C"

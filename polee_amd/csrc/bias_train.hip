// Training of the fragment bias model on the device (src/bias.jl:21-101, :184-399, :464-514, :788-828), and the
// C ABI of both trainers (polee_bias_train_*): `host = 1` in the options runs bias_train_host.cpp instead.  The definitions both share
// are in bias_train_common.hpp; this file is their kernels.  Integer atomics only: every float sum has a fixed order.
#include "bias_train_common.hpp"

#include <rocprim/rocprim.hpp>

using namespace polee;
using namespace polee::biastrain;

namespace {

constexpr int BT_COUNT_BLOCK = 256;
constexpr int BT_LDS_MAXORDER = 5;  // tables up to 2 * 4^6 counters (32 KiB) are privatised in LDS; order 6 adds to global memory

// ---- examples -------------------------------------------------------------------------------------------------------------------
__global__ void bt_examples_kernel(const int64_t *__restrict__ tseq_ptr, const uint8_t *__restrict__ tseq, const int32_t *__restrict__ fg_t,
                                   const int64_t *__restrict__ fg_tpos, const int32_t *__restrict__ fg_fl, const int32_t *__restrict__ bg_t,
                                   const int64_t *__restrict__ bg_tpos_in, const int32_t *__restrict__ bg_fl, int64_t n_fg, int64_t n_bg,
                                   uint64_t seed, uint64_t *__restrict__ left, uint64_t *__restrict__ right, double *__restrict__ gc,
                                   int64_t *__restrict__ bg_pos)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_fg + n_bg) return;
    const bool fg = e < n_fg;
    const int64_t i = fg ? e : e - n_fg;
    int32_t t, fl;
    int64_t tpos;
    if (fg) {
        t = fg_t[i], fl = fg_fl[i], tpos = fg_tpos[i];
    } else if (bg_t) {
        t = bg_t[i], fl = bg_fl[i], tpos = bg_tpos_in[i];
    } else {
        t = fg_t[i], fl = fg_fl[i];
        tpos = bg_tpos(seed, (uint32_t)i, (uint64_t)(tseq_ptr[t + 1] - tseq_ptr[t] - fl + 1));
    }
    if (!fg) bg_pos[i] = tpos;
    make_example(tseq + tseq_ptr[t], tseq_ptr[t + 1] - tseq_ptr[t], tpos, fl, seed, (uint32_t)i, fg ? 1u : 0u, &left[e], &right[e], &gc[e]);
}

// ---- counts and tables ------------------------------------------------------------------------------------------------------------
// cnt: one position's table [2][BT_CLASS], zeroed.  LDS holds [2][cells]; the flush skips counters that stayed zero.
__global__ void bt_count_lds_kernel(const uint64_t *__restrict__ seq, int64_t N, int64_t n_fg, int j, int o, uint32_t *__restrict__ cnt)
{
    extern __shared__ uint32_t bt_lds_cnt[];
    const uint32_t cells = 1u << (2 * (o + 1));
    for (uint32_t k = threadIdx.x; k < 2 * cells; k += blockDim.x) bt_lds_cnt[k] = 0u;
    __syncthreads();
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&bt_lds_cnt[(e < n_fg ? cells : 0u) + cell_of(seq[e], j, o)], 1u);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 2 * cells; k += blockDim.x) {
        const uint32_t v = bt_lds_cnt[k];
        if (v) atomicAdd(&cnt[(k >= cells ? (uint32_t)BT_CLASS + (k - cells) : k)], v);
    }
}
__global__ void bt_count_global_kernel(const uint64_t *__restrict__ seq, int64_t N, int64_t n_fg, int j, int o, uint32_t *__restrict__ cnt)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    atomicAdd(&cnt[(e < n_fg ? (uint32_t)BT_CLASS : 0u) + cell_of(seq[e], j, o)], 1u);
}
__global__ void bt_table_kernel(const uint32_t *__restrict__ cnt, float *__restrict__ ps, int o)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, nctx = 1u << (2 * o);
    if (t >= 2 * nctx) return;
    const uint32_t y = t / nctx, ctx = t % nctx;
    table_row(cnt + y * BT_CLASS, ps + y * BT_CLASS, o, ctx);
}
// seqbias_update_p! for the committed position: its order is the state's
__global__ void bt_commit_kernel(const uint64_t *__restrict__ seq, int64_t N, const SearchState *__restrict__ st, int j,
                                 const float *__restrict__ cur_j, float *__restrict__ fac)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const int o = st->orders[j];
    if (o < 0 || o > BT_MAXORDER || j + o >= BT_K) return;
    const uint32_t cell = cell_of(seq[e], j, o);
    fac[(size_t)j * N + e] = cur_j[cell];
    fac[((size_t)BT_K + j) * N + e] = cur_j[BT_CLASS + cell];
}
__global__ void bt_fill_kernel(float *__restrict__ p, size_t n, float v)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- loss ---------------------------------------------------------------------------------------------------------------------------
// One example per thread, its 40 factors in registers, all eligible candidates and the standing state scored at once; a workgroup is one
// chunk of 256 consecutive examples and leaves 21 partial sums, each by the tree of chunk_tree_sum.  part [21][nchunks].
__global__ void __launch_bounds__(BT_CHUNK) bt_loss_kernel(const uint64_t *__restrict__ seq, int64_t N, int64_t n_fg,
                                                          const SearchState *__restrict__ st, const float *__restrict__ cand,
                                                          const float *__restrict__ fac, double *__restrict__ part, int64_t nchunks)
{
    __shared__ double v[BT_NCAND][BT_CHUNK];
    const int t = threadIdx.x;
    const int64_t e = (int64_t)blockIdx.x * BT_CHUNK + t;
    uint32_t mask = 0;
    for (int j = 0; j < BT_K; ++j) mask |= eligible(st->orders, j) ? 1u << j : 0u;
    double lp[BT_NCAND];
    if (e < N) {
        const uint64_t w = seq[e];
        float f[2][BT_K], cd[2][BT_K];
#pragma unroll
        for (int j = 0; j < BT_K; ++j) {
            f[0][j] = fac[(size_t)j * N + e];
            f[1][j] = fac[((size_t)BT_K + j) * N + e];
            cd[0][j] = cd[1][j] = 1.0f;
            if ((mask >> j) & 1u) {
                const uint32_t cell = cell_of(w, j, st->orders[j] + 1);
                cd[0][j] = cand[(size_t)j * BT_TABLE + cell];
                cd[1][j] = cand[(size_t)j * BT_TABLE + BT_CLASS + cell];
            }
        }
        example_logs(f, cd, mask, e < n_fg, lp);
    } else {
#pragma unroll
        for (int c = 0; c < BT_NCAND; ++c) lp[c] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < BT_NCAND; ++c) v[c][t] = lp[c];
    __syncthreads();
    for (int s = BT_CHUNK / 2; s >= 1; s >>= 1) {
        if (t < s)
            for (int c = 0; c < BT_NCAND; ++c) v[c][t] += v[c][t + s];
        __syncthreads();
    }
    if (t < BT_NCAND) part[(size_t)t * nchunks + blockIdx.x] = v[t][0];
}
// one pass over the partials in index order per candidate, then the decision (score_round, select_round) by thread 0
__global__ void bt_select_kernel(SearchState *__restrict__ st, const double *__restrict__ part, int64_t nchunks, double logn, int init,
                                 int do_select)
{
    __shared__ double sums[BT_NCAND];
    const int t = threadIdx.x;
    if (t < BT_NCAND) {
        // (the adds stay in index order; the loads of 16 partials are issued together, so that a round does not wait for one memory
        // latency per chunk)
        const double *p = part + (size_t)t * nchunks;
        double s = 0.0;
        int64_t ch = 0;
        for (; ch + 16 <= nchunks; ch += 16) {
            double x[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = p[ch + k];
#pragma unroll
            for (int k = 0; k < 16; ++k) s += x[k];
        }
        for (; ch < nchunks; ++ch) s += p[ch];
        sums[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        SearchState s = *st;
        score_round(s, sums, logn, init != 0);
        if (do_select) select_round(s);
        *st = s;
    }
}
__global__ void bt_model_kernel(const float *__restrict__ cur, const SearchState *__restrict__ st, float *__restrict__ ps)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)(BT_K * 4 * BT_CTX)) return;
    ps[i] = model_entry(cur, st->orders, (int)(i / (4 * BT_CTX)), (i / BT_CTX) & 3u, i % BT_CTX);
}

// ---- GC histogram and accuracy ---------------------------------------------------------------------------------------------------------
// (the f32 values sorted are never negative, so their bit patterns sort like them)
__global__ void bt_gc_keys_kernel(const double *__restrict__ gc, int64_t N, uint32_t *__restrict__ keys)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < N) keys[e] = __float_as_uint((float)gc[e]);
}
__global__ void bt_quantile_kernel(const uint32_t *__restrict__ sorted, int64_t N, float *__restrict__ qs)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) gc_quantiles(reinterpret_cast<const float *>(sorted), N, qs);
}
__global__ void bt_gc_bin_kernel(const double *__restrict__ gc, int64_t N, int64_t n_fg, const float *__restrict__ qs, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t c[2 * BT_GC_BINS];
    __shared__ float q[BT_GC_BINS - 1];
    if (threadIdx.x < 2 * BT_GC_BINS) c[threadIdx.x] = 0u;
    if (threadIdx.x < BT_GC_BINS - 1) q[threadIdx.x] = qs[threadIdx.x];
    __syncthreads();
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&c[(e < n_fg ? BT_GC_BINS : 0) + gc_bin_f32(q, (float)gc[e])], 1u);
    __syncthreads();
    if (threadIdx.x < 2 * BT_GC_BINS && c[threadIdx.x]) atomicAdd(&counts[threadIdx.x], c[threadIdx.x]);
}
__global__ void bt_bias_kernel(const uint64_t *__restrict__ left, const uint64_t *__restrict__ right, const double *__restrict__ gc, int64_t N,
                               const float *__restrict__ ps_l, const float *__restrict__ ps_r, const int32_t *__restrict__ orders,
                               const float *__restrict__ expanded, uint32_t *__restrict__ keys)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < N) keys[e] = __float_as_uint(example_bias(ps_l, orders, ps_r, orders + BT_K, expanded, left[e], right[e], gc[e]));
}
__global__ void bt_accuracy_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ sorted, int64_t N, int64_t n_fg,
                                   uint32_t *__restrict__ count)
{
    __shared__ uint32_t c;
    if (threadIdx.x == 0) c = 0u;
    __syncthreads();
    const double med = median_sorted(reinterpret_cast<const float *>(sorted), N);
    uint32_t mine = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (int64_t)gridDim.x * blockDim.x)
        mine += accurate(__uint_as_float(keys[e]), med, e < n_fg) ? 1u : 0u;
    if (mine) atomicAdd(&c, mine);
    __syncthreads();
    if (threadIdx.x == 0 && c) atomicAdd(count, c);
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

}  // namespace

struct polee_bias_train {
    polee_ctx *ctx = nullptr;
    bool host = false;
    uint64_t seed = 0;
    int64_t n_fg = 0, n_bg = 0;
    bool has_bg_pos = false;
    HostTrainer ht;  // host = 1
    Model model;     // host = 0
    DevBuf<uint64_t> d_seq[2];
    DevBuf<double> d_gc, d_part;
    DevBuf<int64_t> d_bg_pos;
    DevBuf<uint32_t> d_cnt, d_keys, d_sorted, d_small;
    DevBuf<float> d_cand, d_cur, d_fac, d_ps[2], d_gcf;
    DevBuf<int32_t> d_orders;
    DevBuf<SearchState> d_state;
    int64_t N() const { return n_fg + n_bg; }
};

namespace {

SearchState fresh_state()
{
    SearchState s;
    memset(&s, 0, sizeof s);
    for (int j = 0; j < BT_K; ++j) {
        s.orders[j] = -1;
        s.losses[j] = INFINITY;
    }
    s.best_j = -1;
    return s;
}

polee_status dev_alloc_work(polee_bias_train *bt)
{
    polee_ctx *ctx = bt->ctx;
    const size_t N = (size_t)bt->N(), nchunks = (N + BT_CHUNK - 1) / BT_CHUNK;
    POLEE_TRY(bt->d_cnt.alloc(ctx, (size_t)BT_K * BT_TABLE));
    POLEE_TRY(bt->d_cand.alloc(ctx, (size_t)BT_K * BT_TABLE));
    POLEE_TRY(bt->d_cur.alloc(ctx, (size_t)BT_K * BT_TABLE));
    POLEE_TRY(bt->d_fac.alloc(ctx, 2 * (size_t)BT_K * N));
    POLEE_TRY(bt->d_part.alloc(ctx, (size_t)BT_NCAND * nchunks));
    POLEE_TRY(bt->d_state.alloc(ctx, 1));
    return POLEE_OK;
}
void dev_free_work(polee_bias_train *bt)
{
    bt->d_cnt.release();
    bt->d_cand.release();
    bt->d_cur.release();
    bt->d_fac.release();
    bt->d_part.release();
}

polee_status dev_reset_side(polee_bias_train *bt, const SearchState &s)
{
    polee_ctx *ctx = bt->ctx;
    const size_t N = (size_t)bt->N();
    POLEE_HIP_TRY(ctx, hipMemsetAsync(bt->d_cand.p, 0, (size_t)BT_K * BT_TABLE * sizeof(float), ctx->stream));
    POLEE_HIP_TRY(ctx, hipMemsetAsync(bt->d_cur.p, 0, (size_t)BT_K * BT_TABLE * sizeof(float), ctx->stream));
    bt_fill_kernel<<<blocks_of((int64_t)(2 * BT_K * N), 256), 256, 0, ctx->stream>>>(bt->d_fac.p, 2 * (size_t)BT_K * N, 1.0f);
    POLEE_KERNEL_CHECK(ctx);
    POLEE_TRY(bt->d_state.upload(ctx, &s, 1));
    return POLEE_OK;
}

polee_status dev_count_table(polee_bias_train *bt, int side, int j, int o)
{
    polee_ctx *ctx = bt->ctx;
    const int64_t N = bt->N();
    uint32_t *cnt = bt->d_cnt.p + (size_t)j * BT_TABLE;
    POLEE_HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (size_t)BT_TABLE * sizeof(uint32_t), ctx->stream));
    if (o <= BT_LDS_MAXORDER) {
        const size_t lds = (size_t)2 * ((size_t)1 << (2 * (o + 1))) * sizeof(uint32_t);
        // (a workgroup counts at least 2048 examples, so that its flush stays the smaller part; at most two workgroups per CU)
        const unsigned grid = std::min<unsigned>(blocks_of(N, BT_COUNT_BLOCK * 8), (unsigned)(2 * ctx->num_cus));
        bt_count_lds_kernel<<<grid, BT_COUNT_BLOCK, lds, ctx->stream>>>(bt->d_seq[side].p, N, bt->n_fg, j, o, cnt);
    } else {
        bt_count_global_kernel<<<blocks_of(N, BT_COUNT_BLOCK), BT_COUNT_BLOCK, 0, ctx->stream>>>(bt->d_seq[side].p, N, bt->n_fg, j, o, cnt);
    }
    POLEE_KERNEL_CHECK(ctx);
    bt_table_kernel<<<blocks_of((int64_t)2 << (2 * o), 256), 256, 0, ctx->stream>>>(cnt, bt->d_cand.p + (size_t)j * BT_TABLE, o);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

polee_status dev_commit(polee_bias_train *bt, int side, int j)
{
    polee_ctx *ctx = bt->ctx;
    const int64_t N = bt->N();
    float *cur_j = bt->d_cur.p + (size_t)j * BT_TABLE;
    POLEE_HIP_TRY(ctx, hipMemcpyAsync(cur_j, bt->d_cand.p + (size_t)j * BT_TABLE, (size_t)BT_TABLE * sizeof(float), hipMemcpyDeviceToDevice,
                                      ctx->stream));
    bt_commit_kernel<<<blocks_of(N, 256), 256, 0, ctx->stream>>>(bt->d_seq[side].p, N, bt->d_state.p, j, cur_j, bt->d_fac.p);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

polee_status dev_round(polee_bias_train *bt, int side, double logn, bool init, bool do_select)
{
    polee_ctx *ctx = bt->ctx;
    const int64_t N = bt->N(), nchunks = (N + BT_CHUNK - 1) / BT_CHUNK;
    bt_loss_kernel<<<(unsigned)nchunks, BT_CHUNK, 0, ctx->stream>>>(bt->d_seq[side].p, N, bt->n_fg, bt->d_state.p, bt->d_cand.p, bt->d_fac.p,
                                                                    bt->d_part.p, nchunks);
    POLEE_KERNEL_CHECK(ctx);
    bt_select_kernel<<<1, 64, 0, ctx->stream>>>(bt->d_state.p, bt->d_part.p, nchunks, logn, init ? 1 : 0, do_select ? 1 : 0);
    POLEE_KERNEL_CHECK(ctx);
    return POLEE_OK;
}

polee_status dev_sort(polee_bias_train *bt, DevScratch &tmp)
{
    polee_ctx *ctx = bt->ctx;
    size_t bytes = 0;
    const size_t N = (size_t)bt->N();
    POLEE_HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, bytes, bt->d_keys.p, bt->d_sorted.p, N, 0, 32, ctx->stream));
    POLEE_HIP_TRY(ctx, tmp.need(bytes));
    POLEE_HIP_TRY(ctx, rocprim::radix_sort_keys(tmp.p, bytes, bt->d_keys.p, bt->d_sorted.p, N, 0, 32, ctx->stream));
    return POLEE_OK;
}

polee_status dev_gc_and_accuracy(polee_bias_train *bt)
{
    polee_ctx *ctx = bt->ctx;
    const int64_t N = bt->N();
    Model &m = bt->model;
    DevScratch tmp(ctx);
    POLEE_TRY(bt->d_keys.alloc(ctx, (size_t)N));
    POLEE_TRY(bt->d_sorted.alloc(ctx, (size_t)N));
    POLEE_TRY(bt->d_small.alloc(ctx, 64));  // counts [30], the accuracy count at [32]
    POLEE_TRY(bt->d_gcf.alloc(ctx, BT_GC_BINS - 1 + BT_GC_EXPANDED));
    POLEE_TRY(bt->d_orders.alloc(ctx, 2 * BT_K));
    float *d_qs = bt->d_gcf.p, *d_bins = bt->d_gcf.p + (BT_GC_BINS - 1);
    const unsigned grid = std::min<unsigned>(blocks_of(N, 256 * 8), (unsigned)(2 * ctx->num_cus));
    POLEE_HIP_TRY(ctx, hipMemsetAsync(bt->d_small.p, 0, 64 * sizeof(uint32_t), ctx->stream));
    bt_gc_keys_kernel<<<blocks_of(N, 256), 256, 0, ctx->stream>>>(bt->d_gc.p, N, bt->d_keys.p);
    POLEE_KERNEL_CHECK(ctx);
    POLEE_TRY(dev_sort(bt, tmp));
    bt_quantile_kernel<<<1, 64, 0, ctx->stream>>>(bt->d_sorted.p, N, d_qs);
    POLEE_KERNEL_CHECK(ctx);
    bt_gc_bin_kernel<<<grid, 256, 0, ctx->stream>>>(bt->d_gc.p, N, bt->n_fg, d_qs, bt->d_small.p);
    POLEE_KERNEL_CHECK(ctx);
    uint32_t counts[2 * BT_GC_BINS];
    POLEE_HIP_TRY(ctx, hipMemcpyAsync(m.gc_qs, d_qs, sizeof m.gc_qs, hipMemcpyDeviceToHost, ctx->stream));
    POLEE_TRY(bt->d_small.download(ctx, counts, 2 * BT_GC_BINS));
    gc_finalize(counts, m.gc_qs, m.gc_bins);
    POLEE_HIP_TRY(ctx, hipMemcpyAsync(d_bins, m.gc_bins, sizeof m.gc_bins, hipMemcpyHostToDevice, ctx->stream));
    POLEE_TRY(bt->d_orders.upload(ctx, &m.orders[0][0], 2 * BT_K));
    bt_bias_kernel<<<blocks_of(N, 256), 256, 0, ctx->stream>>>(bt->d_seq[0].p, bt->d_seq[1].p, bt->d_gc.p, N, bt->d_ps[0].p, bt->d_ps[1].p,
                                                               bt->d_orders.p, d_bins, bt->d_keys.p);
    POLEE_KERNEL_CHECK(ctx);
    POLEE_TRY(dev_sort(bt, tmp));
    bt_accuracy_kernel<<<grid, 256, 0, ctx->stream>>>(bt->d_keys.p, bt->d_sorted.p, N, bt->n_fg, bt->d_small.p + 32);
    POLEE_KERNEL_CHECK(ctx);
    uint32_t acc = 0;
    POLEE_HIP_TRY(ctx, hipMemcpyAsync(&acc, bt->d_small.p + 32, sizeof acc, hipMemcpyDeviceToHost, ctx->stream));
    POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    m.accuracy = (double)acc / (double)N;
    bt->d_keys.release();
    bt->d_sorted.release();
    return POLEE_OK;
}

polee_status dev_finish_side(polee_bias_train *bt, int side)
{
    polee_ctx *ctx = bt->ctx;
    Model &m = bt->model;
    POLEE_TRY(bt->d_ps[side].alloc(ctx, (size_t)BT_K * 4 * BT_CTX));
    bt_model_kernel<<<blocks_of(BT_K * 4 * BT_CTX, 256), 256, 0, ctx->stream>>>(bt->d_cur.p, bt->d_state.p, bt->d_ps[side].p);
    POLEE_KERNEL_CHECK(ctx);
    m.ps[side].resize((size_t)BT_K * 4 * BT_CTX);
    POLEE_HIP_TRY(ctx, hipMemcpyAsync(m.ps[side].data(), bt->d_ps[side].p, m.ps[side].size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    POLEE_TRY(bt->d_state.download(ctx, &m.trace[side], 1));
    std::copy(m.trace[side].orders, m.trace[side].orders + BT_K, m.orders[side]);
    return POLEE_OK;
}

polee_status dev_run(polee_bias_train *bt)
{
    polee_ctx *ctx = bt->ctx;
    const double logn = std::log((double)bt->N());
    POLEE_TRY(dev_alloc_work(bt));
    for (int side = 0; side < 2; ++side) {
        SearchState mirror = fresh_state();  // (the host follows the orders to know which table to count next)
        POLEE_TRY(dev_reset_side(bt, mirror));
        for (int j = 0; j < BT_K; ++j) POLEE_TRY(dev_count_table(bt, side, j, 0));
        for (bool init = true;; init = false) {
            POLEE_TRY(dev_round(bt, side, logn, init, true));
            // the one read of a round: the position the device committed, -1 when the search is over
            int32_t j = -1;
            POLEE_HIP_TRY(ctx, hipMemcpyAsync(&j, &bt->d_state.p->best_j, sizeof j, hipMemcpyDeviceToHost, ctx->stream));
            POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (j < 0 || j >= BT_K) break;
            mirror.orders[j] += 1;
            if (mirror.orders[j] > BT_MAXORDER || j + mirror.orders[j] >= BT_K)
                return fail(ctx, POLEE_ERR_HIP, "polee_bias_train_run: the device committed position %d at order %d", j, mirror.orders[j]);
            POLEE_TRY(dev_commit(bt, side, j));
            if (eligible(mirror.orders, j)) POLEE_TRY(dev_count_table(bt, side, j, mirror.orders[j] + 1));
        }
        POLEE_TRY(dev_finish_side(bt, side));
    }
    dev_free_work(bt);
    POLEE_TRY(dev_gc_and_accuracy(bt));
    bt->model.trained = true;
    return POLEE_OK;
}

polee_status dev_candidates(polee_bias_train *bt, int side, const int32_t *orders_in, double *losses_out, double *loss0_out)
{
    polee_ctx *ctx = bt->ctx;
    const double logn = std::log((double)bt->N());
    POLEE_TRY(dev_alloc_work(bt));
    SearchState s = fresh_state();
    for (int j = 0; j < BT_K; ++j) {
        s.orders[j] = orders_in[j];
        if (orders_in[j] >= 0) s.n_params += (int64_t)1 << (2 * (1 + orders_in[j]));
    }
    POLEE_TRY(dev_reset_side(bt, s));
    for (int j = 0; j < BT_K; ++j) {
        if (s.orders[j] < 0) continue;
        POLEE_TRY(dev_count_table(bt, side, j, s.orders[j]));
        POLEE_TRY(dev_commit(bt, side, j));
    }
    for (int j = 0; j < BT_K; ++j)
        if (eligible(s.orders, j)) POLEE_TRY(dev_count_table(bt, side, j, s.orders[j] + 1));
    POLEE_TRY(dev_round(bt, side, logn, true, false));
    POLEE_TRY(bt->d_state.download(ctx, &s, 1));
    std::copy(s.losses, s.losses + BT_K, losses_out);
    *loss0_out = s.loss0;
    dev_free_work(bt);
    return POLEE_OK;
}

polee_status new_handle(polee_ctx *ctx, const polee_bias_train_opts *opts, const char *who, polee_bias_train **out)
{
    const bool host = opts && opts->host != 0;
    if (!out) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: null output", who);
    *out = nullptr;
    if (!host && !ctx) return fail(nullptr, POLEE_ERR_BAD_ARG, "%s: the device trainer needs a context (or host = 1)", who);
    polee_bias_train *bt = new polee_bias_train();
    bt->host = host;
    bt->ctx = host ? nullptr : ctx;
    bt->seed = opts ? opts->seed : 0;
    if (bt->ctx) ctx_retain(bt->ctx);
    *out = bt;
    return POLEE_OK;
}

}  // namespace

extern "C" {

polee_status polee_bias_train_create(polee_ctx *ctx, int32_t n, const int64_t *tseq_ptr, const uint8_t *tseq, int64_t n_fg,
                                     const int32_t *fg_transcript, const int64_t *fg_tpos, const int32_t *fg_fraglen, int64_t n_bg,
                                     const int32_t *bg_transcript, const int64_t *bg_tpos, const int32_t *bg_fraglen,
                                     const polee_bias_train_opts *opts, polee_bias_train **out)
{
    return host_entry("polee_bias_train_create", [&]() -> polee_status {
        const bool host = opts && opts->host != 0;
        polee_ctx *ectx = host ? nullptr : ctx;
        if (!out) return fail(ectx, POLEE_ERR_BAD_ARG, "polee_bias_train_create: null output");
        *out = nullptr;
        if (!host) POLEE_TRY(use_device(ctx));
        const Inputs in{n, tseq_ptr, tseq, n_fg, fg_transcript, fg_tpos, fg_fraglen, bg_transcript ? n_bg : n_fg, bg_transcript, bg_tpos, bg_fraglen};
        POLEE_TRY(check_inputs(ectx, "polee_bias_train_create", in));
        polee_bias_train *bt = nullptr;
        POLEE_TRY(new_handle(ctx, opts, "polee_bias_train_create", &bt));
        bt->n_fg = in.n_fg;
        bt->n_bg = in.n_bg;
        bt->has_bg_pos = true;
        polee_status s = POLEE_OK;
        if (host) {
            bt->ht.from_fragments(in, bt->seed);
        } else {
            s = [&]() -> polee_status {
                const size_t N = (size_t)bt->N(), total = (size_t)tseq_ptr[n];
                DevBuf<int64_t> d_ptr, d_fpos, d_bpos;
                DevBuf<uint8_t> d_tseq;
                DevBuf<int32_t> d_ft, d_ffl, d_bt, d_bfl;
                POLEE_TRY(d_ptr.upload(ctx, tseq_ptr, (size_t)n + 1));
                POLEE_TRY(d_tseq.upload(ctx, tseq, std::max<size_t>(total, 1)));
                POLEE_TRY(d_ft.upload(ctx, fg_transcript, (size_t)n_fg));
                POLEE_TRY(d_fpos.upload(ctx, fg_tpos, (size_t)n_fg));
                POLEE_TRY(d_ffl.upload(ctx, fg_fraglen, (size_t)n_fg));
                if (bg_transcript) {
                    POLEE_TRY(d_bt.upload(ctx, bg_transcript, (size_t)n_bg));
                    POLEE_TRY(d_bpos.upload(ctx, bg_tpos, (size_t)n_bg));
                    POLEE_TRY(d_bfl.upload(ctx, bg_fraglen, (size_t)n_bg));
                }
                POLEE_TRY(bt->d_seq[0].alloc(ctx, N));
                POLEE_TRY(bt->d_seq[1].alloc(ctx, N));
                POLEE_TRY(bt->d_gc.alloc(ctx, N));
                POLEE_TRY(bt->d_bg_pos.alloc(ctx, (size_t)bt->n_bg));
                bt_examples_kernel<<<blocks_of((int64_t)N, 256), 256, 0, ctx->stream>>>(d_ptr.p, d_tseq.p, d_ft.p, d_fpos.p, d_ffl.p, d_bt.p, d_bpos.p,
                                                                                        d_bfl.p, bt->n_fg, bt->n_bg, bt->seed, bt->d_seq[0].p,
                                                                                        bt->d_seq[1].p, bt->d_gc.p, bt->d_bg_pos.p);
                POLEE_KERNEL_CHECK(ctx);
                POLEE_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                return POLEE_OK;
            }();
        }
        if (s != POLEE_OK) {
            polee_bias_train_destroy(bt);
            return s;
        }
        *out = bt;
        return POLEE_OK;
    });
}

polee_status polee_bias_train_create_from_examples(polee_ctx *ctx, int64_t n_fg, int64_t n_bg, const uint8_t *left_seq, const uint8_t *right_seq,
                                                   const double *frag_gc, const polee_bias_train_opts *opts, polee_bias_train **out)
{
    return host_entry("polee_bias_train_create_from_examples", [&]() -> polee_status {
        const bool host = opts && opts->host != 0;
        polee_ctx *ectx = host ? nullptr : ctx;
        if (!out) return fail(ectx, POLEE_ERR_BAD_ARG, "polee_bias_train_create_from_examples: null output");
        *out = nullptr;
        if (!host) POLEE_TRY(use_device(ctx));
        if (!left_seq || !right_seq || !frag_gc) return fail(ectx, POLEE_ERR_BAD_ARG, "polee_bias_train_create_from_examples: bad argument");
        POLEE_TRY(check_counts(ectx, "polee_bias_train_create_from_examples", n_fg, n_bg));
        for (int64_t e = 0; e < n_fg + n_bg; ++e)
            if (!(frag_gc[e] >= 0.0 && frag_gc[e] <= 1.0))
                return fail(ectx, POLEE_ERR_BAD_ARG, "polee_bias_train_create_from_examples: frag_gc[%lld] is not in 0 .. 1", (long long)e);
        polee_bias_train *bt = nullptr;
        POLEE_TRY(new_handle(ctx, opts, "polee_bias_train_create_from_examples", &bt));
        bt->n_fg = n_fg;
        bt->n_bg = n_bg;
        // (packing 40 codes per example is the host's in both trainers: the examples arrive as host arrays)
        bt->ht.from_examples(n_fg, n_bg, left_seq, right_seq, frag_gc);
        if (!host) {
            polee_status s = [&]() -> polee_status {
                POLEE_TRY(bt->d_seq[0].upload(ctx, bt->ht.seq[0]));
                POLEE_TRY(bt->d_seq[1].upload(ctx, bt->ht.seq[1]));
                POLEE_TRY(bt->d_gc.upload(ctx, bt->ht.gc));
                return POLEE_OK;
            }();
            bt->ht = HostTrainer();
            if (s != POLEE_OK) {
                polee_bias_train_destroy(bt);
                return s;
            }
        }
        *out = bt;
        return POLEE_OK;
    });
}

void polee_bias_train_destroy(polee_bias_train *bt)
{
    if (!bt) return;
    polee_ctx *ctx = bt->ctx;
    if (ctx) (void)hipSetDevice(ctx->device);
    delete bt;
    if (ctx) ctx_release(ctx);
}

polee_status polee_bias_train_run(polee_bias_train *bt)
{
    return entry(bt, "polee_bias_train_run", [&](polee_ctx *ctx) -> polee_status {
        if (bt->host) {
            bt->ht.run();
            return POLEE_OK;
        }
        const polee_status s = dev_run(bt);
        if (s != POLEE_OK) dev_free_work(bt);
        return s;
    });
}

polee_status polee_bias_train_candidates(polee_bias_train *bt, int32_t side, const int32_t *orders_in, double *losses_out, double *loss0_out)
{
    return entry(bt, "polee_bias_train_candidates", [&](polee_ctx *ctx) -> polee_status {
        if ((side != 0 && side != 1) || !orders_in || !losses_out || !loss0_out)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_bias_train_candidates: bad argument");
        for (int j = 0; j < BT_K; ++j)
            if (orders_in[j] < -1 || orders_in[j] > BT_MAXORDER || (orders_in[j] >= 0 && j + orders_in[j] >= BT_K))
                return fail(ctx, POLEE_ERR_BAD_ARG, "polee_bias_train_candidates: order %d at position %d", orders_in[j], j + 1);
        if (bt->host) {
            bt->ht.candidates(side, orders_in, losses_out, loss0_out);
            return POLEE_OK;
        }
        const polee_status s = dev_candidates(bt, side, orders_in, losses_out, loss0_out);
        if (s != POLEE_OK) dev_free_work(bt);
        return s;
    });
}

polee_status polee_bias_train_get_model(polee_bias_train *bt, int32_t *orders_left, int32_t *orders_right, float *ps_left, float *ps_right,
                                        float *gc_bins, float *gc_qs, double *accuracy)
{
    return entry(bt, "polee_bias_train_get_model", [&](polee_ctx *ctx) -> polee_status {
        const Model &m = bt->host ? bt->ht.model : bt->model;
        if (!m.trained) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_bias_train_get_model: polee_bias_train_run has not completed");
        if (orders_left) std::copy(m.orders[0], m.orders[0] + BT_K, orders_left);
        if (orders_right) std::copy(m.orders[1], m.orders[1] + BT_K, orders_right);
        if (ps_left) std::copy(m.ps[0].begin(), m.ps[0].end(), ps_left);
        if (ps_right) std::copy(m.ps[1].begin(), m.ps[1].end(), ps_right);
        if (gc_bins) std::copy(m.gc_bins, m.gc_bins + BT_GC_EXPANDED, gc_bins);
        if (gc_qs) std::copy(m.gc_qs, m.gc_qs + BT_GC_BINS - 1, gc_qs);
        if (accuracy) *accuracy = m.accuracy;
        return POLEE_OK;
    });
}

polee_status polee_bias_train_get_examples(polee_bias_train *bt, int64_t *n_fg, int64_t *n_bg, uint64_t *left, uint64_t *right, double *frag_gc,
                                           int64_t *bg_tpos)
{
    return entry(bt, "polee_bias_train_get_examples", [&](polee_ctx *ctx) -> polee_status {
        const size_t N = (size_t)bt->N();
        if (n_fg) *n_fg = bt->n_fg;
        if (n_bg) *n_bg = bt->n_bg;
        if (bg_tpos && !bt->has_bg_pos)
            return fail(ctx, POLEE_ERR_BAD_ARG, "polee_bias_train_get_examples: a trainer made from examples has no positions");
        if (bt->host) {
            if (left) std::copy(bt->ht.seq[0].begin(), bt->ht.seq[0].end(), left);
            if (right) std::copy(bt->ht.seq[1].begin(), bt->ht.seq[1].end(), right);
            if (frag_gc) std::copy(bt->ht.gc.begin(), bt->ht.gc.end(), frag_gc);
            if (bg_tpos) std::copy(bt->ht.bg_pos.begin(), bt->ht.bg_pos.end(), bg_tpos);
            return POLEE_OK;
        }
        if (left) POLEE_TRY(bt->d_seq[0].download(ctx, left, N));
        if (right) POLEE_TRY(bt->d_seq[1].download(ctx, right, N));
        if (frag_gc) POLEE_TRY(bt->d_gc.download(ctx, frag_gc, N));
        if (bg_tpos) POLEE_TRY(bt->d_bg_pos.download(ctx, bg_tpos, (size_t)bt->n_bg));
        return POLEE_OK;
    });
}

polee_status polee_bias_train_get_trace(polee_bias_train *bt, int32_t side, int32_t *rounds, int32_t *positions, double *losses)
{
    return entry(bt, "polee_bias_train_get_trace", [&](polee_ctx *ctx) -> polee_status {
        const Model &m = bt->host ? bt->ht.model : bt->model;
        if (side != 0 && side != 1) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_bias_train_get_trace: side must be 0 (left) or 1 (right)");
        if (!m.trained) return fail(ctx, POLEE_ERR_BAD_ARG, "polee_bias_train_get_trace: polee_bias_train_run has not completed");
        const SearchState &s = m.trace[side];
        if (rounds) *rounds = s.rounds;
        if (positions) std::copy(s.trace_j, s.trace_j + s.rounds, positions);
        if (losses) std::copy(s.trace, s.trace + s.rounds + 1, losses);
        return POLEE_OK;
    });
}

}  // extern "C"

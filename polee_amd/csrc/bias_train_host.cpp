// The bias model trainer on the host: the definitions of bias_train_common.hpp step by step, examples in
// parallel over POLEE_HOST_THREADS.  It is what `host = 1` runs, and the tests hold the device trainer (bias_train.hip) against it bit
// for bit.  No context, no device.
#include "bias_train_common.hpp"

#include <algorithm>

namespace polee {
namespace biastrain {

polee_status check_counts(polee_ctx *ctx, const char *who, int64_t n_fg, int64_t n_bg)
{
    if (n_fg < 1 || n_bg < 1) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: needs foreground and background examples", who);
    if (n_fg + n_bg < BT_MIN_EXAMPLES)
        return fail(ctx, POLEE_ERR_BAD_ARG, "%s: %lld examples; the GC quantiles need at least %lld", who, (long long)(n_fg + n_bg),
                    (long long)BT_MIN_EXAMPLES);
    if (n_fg + n_bg >= BT_MAX_EXAMPLES)
        return fail(ctx, POLEE_ERR_UNSUPPORTED, "%s: %lld examples; counts stay exact in f32 below 2^24", who, (long long)(n_fg + n_bg));
    return POLEE_OK;
}

static polee_status check_list(polee_ctx *ctx, const char *who, const char *what, const Inputs &in, int64_t cnt, const int32_t *t,
                               const int64_t *tpos, const int32_t *fl)
{
    for (int64_t i = 0; i < cnt; ++i) {
        if (t[i] < 0 || t[i] >= in.n) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: %s fragment %lld: transcript %d", who, what, (long long)i, t[i]);
        const int64_t tlen = in.tseq_ptr[t[i] + 1] - in.tseq_ptr[t[i]];
        if (fl[i] < BT_K) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: %s fragment %lld: fraglen %d < %d", who, what, (long long)i, fl[i], BT_K);
        if (tpos && (tpos[i] < 1 || tpos[i] + fl[i] - 1 > tlen))
            return fail(ctx, POLEE_ERR_BAD_ARG, "%s: %s fragment %lld: positions %lld .. %lld of a transcript of %lld", who, what,
                        (long long)i, (long long)tpos[i], (long long)(tpos[i] + fl[i] - 1), (long long)tlen);
        if (!tpos && fl[i] > tlen)
            return fail(ctx, POLEE_ERR_BAD_ARG, "%s: %s fragment %lld: fraglen %d in a transcript of %lld", who, what, (long long)i, fl[i],
                        (long long)tlen);
    }
    return POLEE_OK;
}

polee_status check_inputs(polee_ctx *ctx, const char *who, const Inputs &in)
{
    if (in.n < 1 || !in.tseq_ptr || !in.tseq || !in.fg_t || !in.fg_tpos || !in.fg_fl)
        return fail(ctx, POLEE_ERR_BAD_ARG, "%s: bad argument", who);
    if (in.bg_t && (!in.bg_tpos || !in.bg_fl)) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: the background list is incomplete", who);
    if (!in.bg_t && in.n_bg != in.n_fg)
        return fail(ctx, POLEE_ERR_BAD_ARG, "%s: a drawn background has one fragment per foreground fragment", who);
    POLEE_TRY(check_counts(ctx, who, in.n_fg, in.n_bg));
    if (in.tseq_ptr[0] != 0) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: tseq_ptr[0] != 0", who);
    for (int32_t j = 0; j < in.n; ++j) {
        const int64_t tlen = in.tseq_ptr[j + 1] - in.tseq_ptr[j];
        if (tlen < 0 || tlen > INT32_MAX) return fail(ctx, POLEE_ERR_BAD_ARG, "%s: transcript %d has length %lld", who, j, (long long)tlen);
    }
    POLEE_TRY(check_list(ctx, who, "foreground", in, in.n_fg, in.fg_t, in.fg_tpos, in.fg_fl));
    if (in.bg_t) POLEE_TRY(check_list(ctx, who, "background", in, in.n_bg, in.bg_t, in.bg_tpos, in.bg_fl));
    return POLEE_OK;
}

void HostTrainer::from_fragments(const Inputs &in, uint64_t seed_)
{
    n_fg = in.n_fg;
    n_bg = in.n_bg;
    seed = seed_;
    const size_t Nn = (size_t)N();
    seq[0].assign(Nn, 0);
    seq[1].assign(Nn, 0);
    gc.assign(Nn, 0.0);
    bg_pos.assign((size_t)n_bg, 0);
    parallel_chunks(Nn, 4096, [&](size_t lo, size_t hi, unsigned) {
        for (size_t e = lo; e < hi; ++e) {
            const bool fg = (int64_t)e < n_fg;
            const size_t i = fg ? e : e - (size_t)n_fg;
            int32_t t, fl;
            int64_t tpos;
            if (fg) {
                t = in.fg_t[i], fl = in.fg_fl[i], tpos = in.fg_tpos[i];
            } else if (in.bg_t) {
                t = in.bg_t[i], fl = in.bg_fl[i], tpos = in.bg_tpos[i];
            } else {
                t = in.fg_t[i], fl = in.fg_fl[i];
                tpos = bg_tpos(seed, (uint32_t)i, (uint64_t)(in.tseq_ptr[t + 1] - in.tseq_ptr[t] - fl + 1));
            }
            if (!fg) bg_pos[i] = tpos;
            make_example(in.tseq + in.tseq_ptr[t], in.tseq_ptr[t + 1] - in.tseq_ptr[t], tpos, fl, seed, (uint32_t)i, fg ? 1u : 0u,
                         &seq[0][e], &seq[1][e], &gc[e]);
        }
    });
    model = Model();
}

void HostTrainer::from_examples(int64_t n_fg_, int64_t n_bg_, const uint8_t *left, const uint8_t *right, const double *frag_gc)
{
    n_fg = n_fg_;
    n_bg = n_bg_;
    seed = 0;
    const size_t Nn = (size_t)N();
    seq[0].assign(Nn, 0);
    seq[1].assign(Nn, 0);
    gc.assign(frag_gc, frag_gc + Nn);
    bg_pos.clear();
    for (size_t e = 0; e < Nn; ++e)
        for (int k = 0; k < BT_K; ++k) {
            const uint32_t a = left[e * BT_K + k], b = right[e * BT_K + k];
            seq[0][e] = (seq[0][e] << 2) | (a > 3u ? 0u : a);
            seq[1][e] = (seq[1][e] << 2) | (b > 3u ? 0u : b);
        }
    model = Model();
}

void HostTrainer::reset_side()
{
    const size_t Nn = (size_t)N();
    cnt.assign((size_t)BT_K * BT_TABLE, 0);
    cand.assign((size_t)BT_K * BT_TABLE, 0.0f);
    cur.assign((size_t)BT_K * BT_TABLE, 0.0f);
    fac.assign(2 * (size_t)BT_K * Nn, 1.0f);
    st = SearchState();
    for (int j = 0; j < BT_K; ++j) {
        st.orders[j] = -1;
        st.losses[j] = INFINITY;
    }
    st.best_j = -1;
    st.rounds = 0;
    st.n_params = 0;
    st.loss0 = 0.0;
}

// the counts and the table of position j under order o (seqbias_update_param_estimate!)
void HostTrainer::count_table(int side, int j, int o)
{
    const size_t Nn = (size_t)N();
    uint32_t *c = cnt.data() + (size_t)j * BT_TABLE;
    std::fill(c, c + BT_TABLE, 0u);
    std::mutex mu;
    const uint32_t cells = 1u << (2 * (o + 1));
    parallel_chunks(Nn, 65536, [&](size_t lo, size_t hi, unsigned) {
        std::vector<uint32_t> mine(2 * (size_t)cells, 0u);
        for (size_t e = lo; e < hi; ++e) ++mine[((int64_t)e < n_fg ? cells : 0u) + cell_of(seq[side][e], j, o)];
        std::lock_guard<std::mutex> g(mu);
        for (uint32_t k = 0; k < cells; ++k) {
            c[k] += mine[k];
            c[BT_CLASS + k] += mine[cells + k];
        }
    });
    float *p = cand.data() + (size_t)j * BT_TABLE;
    for (int y = 0; y < 2; ++y)
        for (uint32_t ctx = 0; ctx < (1u << (2 * o)); ++ctx) table_row(c + y * BT_CLASS, p + y * BT_CLASS, o, ctx);
}

// the candidate of position j becomes the model's: the table and every example's factor (seqbias_update_p!); st.orders[j] is the new order
void HostTrainer::commit(int side, int j)
{
    const size_t Nn = (size_t)N();
    const int o = st.orders[j];
    std::copy(cand.begin() + (size_t)j * BT_TABLE, cand.begin() + (size_t)(j + 1) * BT_TABLE, cur.begin() + (size_t)j * BT_TABLE);
    const float *p = cur.data() + (size_t)j * BT_TABLE;
    parallel_chunks(Nn, 65536, [&](size_t lo, size_t hi, unsigned) {
        for (size_t e = lo; e < hi; ++e) {
            const uint32_t cell = cell_of(seq[side][e], j, o);
            fac[(size_t)j * Nn + e] = p[cell];
            fac[((size_t)BT_K + j) * Nn + e] = p[BT_CLASS + cell];
        }
    });
}

void HostTrainer::losses(int side, double *sums)
{
    const size_t Nn = (size_t)N(), nchunks = (Nn + BT_CHUNK - 1) / BT_CHUNK;
    std::vector<double> part((size_t)BT_NCAND * nchunks);
    uint32_t mask = 0;
    for (int j = 0; j < BT_K; ++j) mask |= eligible(st.orders, j) ? 1u << j : 0u;
    parallel_chunks(nchunks, 16, [&](size_t lo, size_t hi, unsigned) {
        std::vector<double> v((size_t)BT_NCAND * BT_CHUNK);
        for (size_t ch = lo; ch < hi; ++ch) {
            std::fill(v.begin(), v.end(), 0.0);
            for (size_t t = 0; t < (size_t)BT_CHUNK && ch * BT_CHUNK + t < Nn; ++t) {
                const size_t e = ch * BT_CHUNK + t;
                float f[2][BT_K], cd[2][BT_K];
                for (int j = 0; j < BT_K; ++j) {
                    f[0][j] = fac[(size_t)j * Nn + e];
                    f[1][j] = fac[((size_t)BT_K + j) * Nn + e];
                    cd[0][j] = cd[1][j] = 1.0f;
                    if ((mask >> j) & 1u) {
                        const uint32_t cell = cell_of(seq[side][e], j, st.orders[j] + 1);
                        cd[0][j] = cand[(size_t)j * BT_TABLE + cell];
                        cd[1][j] = cand[(size_t)j * BT_TABLE + BT_CLASS + cell];
                    }
                }
                double lp[BT_NCAND];
                example_logs(f, cd, mask, (int64_t)e < n_fg, lp);
                for (int c = 0; c < BT_NCAND; ++c) v[(size_t)c * BT_CHUNK + t] = lp[c];
            }
            for (int c = 0; c < BT_NCAND; ++c) part[(size_t)c * nchunks + ch] = chunk_tree_sum(v.data() + (size_t)c * BT_CHUNK);
        }
    });
    for (int c = 0; c < BT_NCAND; ++c) {
        double s = 0.0;
        for (size_t ch = 0; ch < nchunks; ++ch) s += part[(size_t)c * nchunks + ch];
        sums[c] = s;
    }
}

void HostTrainer::finish_side(int side)
{
    std::copy(st.orders, st.orders + BT_K, model.orders[side]);
    model.ps[side].assign((size_t)BT_K * 4 * BT_CTX, 1.0f);
    for (int j = 0; j < BT_K; ++j)
        for (uint32_t nt = 0; nt < 4; ++nt)
            for (uint32_t ctx = 0; ctx < (uint32_t)BT_CTX; ++ctx)
                model.ps[side][((size_t)j * 4 + nt) * BT_CTX + ctx] = model_entry(cur.data(), st.orders, j, nt, ctx);
    model.trace[side] = st;
}

void HostTrainer::gc_and_accuracy()
{
    const size_t Nn = (size_t)N();
    std::vector<float> x(Nn), sorted;
    for (size_t e = 0; e < Nn; ++e) x[e] = (float)gc[e];
    sorted = x;
    std::sort(sorted.begin(), sorted.end());
    gc_quantiles(sorted.data(), (int64_t)Nn, model.gc_qs);
    uint32_t counts[2 * BT_GC_BINS] = {0};
    for (size_t e = 0; e < Nn; ++e) ++counts[((int64_t)e < n_fg ? BT_GC_BINS : 0) + gc_bin_f32(model.gc_qs, x[e])];
    gc_finalize(counts, model.gc_qs, model.gc_bins);
    parallel_chunks(Nn, 65536, [&](size_t lo, size_t hi, unsigned) {
        for (size_t e = lo; e < hi; ++e)
            x[e] = example_bias(model.ps[0].data(), model.orders[0], model.ps[1].data(), model.orders[1], model.gc_bins, seq[0][e], seq[1][e],
                                gc[e]);
    });
    sorted = x;
    std::sort(sorted.begin(), sorted.end());
    const double med = median_sorted(sorted.data(), (int64_t)Nn);
    int64_t acc = 0;
    for (size_t e = 0; e < Nn; ++e) acc += accurate(x[e], med, (int64_t)e < n_fg) ? 1 : 0;
    model.accuracy = (double)acc / (double)Nn;
}

void HostTrainer::run()
{
    const double logn = std::log((double)N());
    for (int side = 0; side < 2; ++side) {
        reset_side();
        for (int j = 0; j < BT_K; ++j) count_table(side, j, 0);
        for (bool init = true;; init = false) {
            double sums[BT_NCAND];
            losses(side, sums);
            score_round(st, sums, logn, init);
            select_round(st);
            const int j = st.best_j;
            if (j < 0) break;
            commit(side, j);
            if (eligible(st.orders, j)) count_table(side, j, st.orders[j] + 1);
        }
        finish_side(side);
    }
    gc_and_accuracy();
    model.trained = true;
    cnt = std::vector<uint32_t>();
    cand = cur = fac = std::vector<float>();
}

void HostTrainer::candidates(int side, const int32_t *orders_in, double *losses_out, double *loss0_out)
{
    const double logn = std::log((double)N());
    reset_side();
    for (int j = 0; j < BT_K; ++j) {
        const int o = orders_in[j];
        if (o < 0) continue;
        count_table(side, j, o);
        st.orders[j] = o;
        st.n_params += (int64_t)1 << (2 * (1 + o));
        commit(side, j);
    }
    for (int j = 0; j < BT_K; ++j)
        if (eligible(st.orders, j)) count_table(side, j, st.orders[j] + 1);
    double sums[BT_NCAND];
    losses(side, sums);
    score_round(st, sums, logn, true);
    std::copy(st.losses, st.losses + BT_K, losses_out);
    *loss0_out = st.loss0;
    cnt = std::vector<uint32_t>();
    cand = cur = fac = std::vector<float>();
}

}  // namespace biastrain
}  // namespace polee

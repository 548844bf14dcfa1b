// Training of the fragment bias model (src/bias.jl:21-101, :184-399, :464-514, :788-828): the definitions that
// the device trainer (bias_train.hip), the host trainer (bias_train_host.cpp) and the NumPy restatement of the tests share.  Everything
// here is integers, Philox counters and IEEE operations one rounding at a time (both sources are compiled with -ffp-contract=off), so
// host and device give the same model bit for bit; only log() differs, by its ulp error, and only the loss trace sees that.
#pragma once
#include "common.hpp"
#include "rng.hpp"

#include <cmath>

namespace polee {
namespace biastrain {

constexpr int BT_K = 20;            // positions per fragment end: BIAS_SEQ_OUTER_CTX + BIAS_SEQ_INNER_CTX (constants.jl)
constexpr int BT_OUTER = 5;         // BIAS_SEQ_OUTER_CTX
constexpr int BT_MAXORDER = 6;      // bias.jl:273
constexpr int BT_CTX = 4096;        // 4^maxorder
constexpr int BT_CLASS = 4 * BT_CTX;  // one class of one position's table: [nt][ctx] packed as nt << 2 order | ctx
constexpr int BT_TABLE = 2 * BT_CLASS;  // one position's table: [class][nt << 2 order | ctx], class 0 background, 1 foreground
constexpr int BT_MAX_ROUNDS = BT_K * (BT_MAXORDER + 1);
constexpr int BT_CHUNK = 256;       // examples per partial sum of the loss
constexpr int BT_NCAND = BT_K + 1;  // the 20 candidates and, last, the state as it stands
constexpr int BT_GC_BINS = 15, BT_GC_EXPANDED = 100;  // bias.jl:473, :506
constexpr int64_t BT_MIN_EXAMPLES = 30, BT_MAX_EXAMPLES = (int64_t)1 << 24;
constexpr uint32_t BT_TAG_PAD = 0x62706164u;  // "bpad"
constexpr uint32_t BT_TAG_BG = 0x62626764u;   // "bbgd"

// A nucleotide beyond a transcript's end (randdna, bias.jl:83-101): counter (example index within its class, class, offset in the
// padded fragment, tag), the low two bits of the block's first word.
__host__ __device__ inline uint32_t pad_nt(uint64_t seed, uint32_t i, uint32_t cls, uint32_t off)
{
    uint32_t c[4] = {i, cls, off, BT_TAG_PAD};
    philox4x32_10(c, seed);
    return c[0] & 3u;
}
// The position of background fragment i: uniform in 1 .. span (fragmodel.jl:243), span = tlen - fraglen + 1 < 2^32.
__host__ __device__ inline int64_t bg_tpos(uint64_t seed, uint32_t i, uint64_t span)
{
    uint32_t c[4] = {i, 0u, 0u, BT_TAG_BG};
    philox4x32_10(c, seed);
    return 1 + (int64_t)(((uint64_t)c[0] * span) >> 32);
}

// BiasTrainingExample(tseq, tpos, fl) (bias.jl:21-80) without the unused a_freqs .. t_freqs.  ts: the transcript's codes; each end is
// 20 two-bit codes in one word, position 1 in bits 39:38, position 20 in bits 1:0.
__host__ __device__ inline void make_example(const uint8_t *ts, int64_t tlen, int64_t tpos, int32_t fl, uint64_t seed, uint32_t i,
                                             uint32_t cls, uint64_t *left, uint64_t *right, double *gc)
{
    uint64_t l = 0, r = 0;
    for (int k = 0; k < 2 * BT_K; ++k) {
        const int64_t off = k < BT_K ? k : (int64_t)fl + 2 * BT_OUTER - 2 * BT_K + k;  // offset in the padded fragment
        const int64_t p = tpos - BT_OUTER + off;                                       // 1-based transcript position
        uint32_t c;
        if (p < 1 || p > tlen) {
            c = pad_nt(seed, i, cls, (uint32_t)off);
        } else {
            c = ts[p - 1];
            c = c > 3u ? 0u : c;  // nt2bit: N -> A
        }
        if (k < BT_K)
            l = (l << 2) | c;
        else
            r = (r << 2) | c;
    }
    int32_t g = 0;
    for (int64_t p = tpos; p < tpos + fl; ++p) g += (ts[p - 1] == 1u || ts[p - 1] == 2u) ? 1 : 0;
    *left = l;
    *right = r;
    *gc = (double)g / (double)fl;
}

// nt << 2 o | ctx of position j (0-based) under order o: the base at j and the o bases after it, the base at j+1 the context's most
// significant digit (ctx = (ctx << 2) | seq[j+l], bias.jl:188-191)
__host__ __device__ inline uint32_t cell_of(uint64_t w, int j, int o)
{
    return (uint32_t)(w >> (2 * (BT_K - 1 - j - o))) & ((1u << (2 * (o + 1))) - 1u);
}
__host__ __device__ inline bool eligible(const int32_t *orders, int j) { return orders[j] < BT_MAXORDER && j + 1 + orders[j] < BT_K; }
__host__ __device__ inline int64_t added_params(int o) { return ((int64_t)1 << (2 * (1 + o))) - (o == 0 ? 0 : ((int64_t)1 << (2 * o))); }

// seqbias_update_param_estimate! (bias.jl:184-201) for one (class, ctx): the four entries (1 + count) / z in f32
__host__ __device__ inline void table_row(const uint32_t *cnt, float *ps, int o, uint32_t ctx)
{
    float a[4];
    for (uint32_t nt = 0; nt < 4; ++nt) a[nt] = 1.0f + (float)cnt[(nt << (2 * o)) | ctx];
    const float z = ((a[0] + a[1]) + a[2]) + a[3];
    for (uint32_t nt = 0; nt < 4; ++nt) ps[(nt << (2 * o)) | ctx] = a[nt] / z;
}

// compute_seqbias_loss's term of one example (bias.jl:246-255) for the 20 candidates and for the state as it stands: f [class][j] are
// the current factors, cand [class][j] the candidate's factor of every eligible position (mask).  The log is taken in f64.
__host__ __device__ inline void example_logs(const float (&f)[2][BT_K], const float (&cand)[2][BT_K], uint32_t mask, bool y,
                                             double (&lp)[BT_NCAND])
{
    for (int c = 0; c < BT_NCAND; ++c) {
        if (c < BT_K && !((mask >> c) & 1u)) {
            lp[c] = 0.0;
            continue;
        }
        float p_fg = 1.0f, p_bg = 1.0f;
        for (int j = 0; j < BT_K; ++j) {
            p_fg *= j == c ? cand[1][j] : f[1][j];
            p_bg *= j == c ? cand[0][j] : f[0][j];
        }
        const float p = p_fg / (p_fg + p_bg);
        const float q = y ? p : 1.0f - p;
        lp[c] = log((double)q);
    }
}

// The state of one side's search (bias.jl:349-396); it lives on the device in the device trainer.
struct SearchState {
    int32_t orders[BT_K];
    int32_t best_j;  // the position the last round committed, -1: none (the search is over)
    int32_t rounds;  // committed rounds
    int64_t n_params;
    double loss0;
    double losses[BT_K];
    double trace[BT_MAX_ROUNDS + 1];  // loss0 at the start and after every committed round
    int32_t trace_j[BT_MAX_ROUNDS];
};

// sums [21]: the log-likelihoods.  init: loss0 is taken from the state as it stands (bias.jl:352)
__host__ __device__ inline void score_round(SearchState &s, const double *sums, double logn, bool init)
{
    if (init) {
        s.loss0 = -(2.0 * sums[BT_K] - (double)s.n_params * logn);
        s.trace[0] = s.loss0;
    }
    for (int j = 0; j < BT_K; ++j)
        s.losses[j] = eligible(s.orders, j) ? -(2.0 * sums[j] - (double)(s.n_params + added_params(s.orders[j] + 1)) * logn) : INFINITY;
}
// the ascending scan with < (bias.jl:357-395): the smallest loss, the lowest j among equal ones, a NaN never wins
__host__ __device__ inline void select_round(SearchState &s)
{
    double best = s.loss0;
    int bj = -1;
    for (int j = 0; j < BT_K; ++j)
        if (s.losses[j] < best) {
            best = s.losses[j];
            bj = j;
        }
    s.best_j = bj;
    if (bj < 0 || s.rounds >= BT_MAX_ROUNDS) {
        s.best_j = -1;
        return;
    }
    s.orders[bj] += 1;
    s.n_params += added_params(s.orders[bj]);
    s.loss0 = best;
    s.trace_j[s.rounds] = bj;
    s.rounds += 1;
    s.trace[s.rounds] = best;
}

// ps[j][nt][ctx] of the finished model (bias.jl:398): foreground over background where the model reads, 1 elsewhere
__host__ __device__ inline float model_entry(const float *cur /*[20][BT_TABLE]*/, const int32_t *orders, int j, uint32_t nt, uint32_t ctx)
{
    const int o = orders[j];
    if (o < 0 || ctx >= (1u << (2 * o))) return 1.0f;
    const uint32_t cell = (nt << (2 * o)) | ctx;
    return cur[(size_t)j * BT_TABLE + BT_CLASS + cell] / cur[(size_t)j * BT_TABLE + cell];
}
// evaluate(sb, seq) (bias.jl:402-416) on a packed end
__host__ __device__ inline float model_eval(const float *ps /*[20][4][4096]*/, const int32_t *orders, uint64_t w)
{
    float bias = 1.0f;
    for (int j = 0; j < BT_K; ++j) {
        const int o = orders[j];
        if (o < 0) continue;
        const uint32_t cell = cell_of(w, j, o);
        bias *= ps[((size_t)j * 4 + (cell >> (2 * o))) * BT_CTX + (cell & ((1u << (2 * o)) - 1u))];
    }
    return bias;
}

// The 14 quantile boundaries (bias.jl:476-489) of the sorted f32 xs [n], n >= 30: with unit weights the running sum at element i
// (1-based) is i, so boundary k is taken at the first i > f32(k binsize) that lies after boundary k-1's element.
__host__ __device__ inline void gc_quantiles(const float *sorted, int64_t n, float *qs)
{
    const float binsize = (float)n / (float)BT_GC_BINS;
    int64_t prev = 0;
    for (int k = 1; k < BT_GC_BINS; ++k) {
        const double thr = (double)((float)k * binsize);
        int64_t i = (int64_t)floor(thr) + 1;
        if (i <= prev) i = prev + 1;
        if (i > n) i = n;  // (cannot happen for n >= 30)
        qs[k - 1] = sorted[i - 1];
        prev = i;
    }
}
// searchsorted(qs, x).start - 1 (0-based bin) for an f32 x
__host__ __device__ inline int gc_bin_f32(const float *qs, float x)
{
    int b = 0;
    for (int k = 0; k < BT_GC_BINS - 1; ++k) b += qs[k] < x ? 1 : 0;
    return b;
}
// counts [2][15] -> the 100 expanded bins (bias.jl:491-511)
inline void gc_finalize(const uint32_t *counts, const float *qs, float *expanded)
{
    float c[2][BT_GC_BINS], s[2] = {0.0f, 0.0f}, bins[BT_GC_BINS];
    for (int y = 0; y < 2; ++y)
        for (int b = 0; b < BT_GC_BINS; ++b) {
            c[y][b] = 1.0f + (float)counts[y * BT_GC_BINS + b];
            s[y] += c[y][b];
        }
    for (int b = 0; b < BT_GC_BINS; ++b) bins[b] = (c[1][b] / s[1]) / (c[0][b] / s[0]);
    for (int i = 1; i <= BT_GC_EXPANDED; ++i) {
        const double q = ((double)i - 0.5) / (double)BT_GC_EXPANDED;
        int b = 0;
        for (int k = 0; k < BT_GC_BINS - 1; ++k) b += (double)qs[k] < q ? 1 : 0;
        expanded[i - 1] = bins[b];
    }
}
// evaluate(hist, x) (bias.jl:517-520), round half to even as xb_hist_f64 (xbuild.hip)
__host__ __device__ inline float gc_eval(const float *expanded, double x)
{
    long long i = (long long)rint(x * (double)BT_GC_EXPANDED);
    i = i < 1 ? 1 : (i > BT_GC_EXPANDED ? BT_GC_EXPANDED : i);
    return expanded[i - 1];
}
// the bias of one example as accuracy() computes it (bias.jl:798-803), an f32
__host__ __device__ inline float example_bias(const float *ps_l, const int32_t *ord_l, const float *ps_r, const int32_t *ord_r,
                                              const float *expanded, uint64_t l, uint64_t r, double gc)
{
    return ((model_eval(ps_l, ord_l, l) * model_eval(ps_r, ord_r, r)) * gc_eval(expanded, gc)) * 1.0f;
}
// median(bs) of the sorted values, n >= 1 (Statistics.middle: x/2 + y/2)
__host__ __device__ inline double median_sorted(const float *sorted, int64_t n)
{
    if (n & 1) return (double)sorted[n / 2];
    return (double)sorted[n / 2 - 1] / 2.0 + (double)sorted[n / 2] / 2.0;
}
__host__ __device__ inline bool accurate(float b, double med, bool y)
{
    const double d = (double)b - med;
    return y ? d > 0.0 : d <= 0.0;
}

// the tree that sums the 256 terms of a chunk: v[t] += v[t + s] for s = 128, 64, .. 1 (the device does it in LDS)
inline double chunk_tree_sum(double *v)
{
    for (int s = BT_CHUNK / 2; s >= 1; s >>= 1)
        for (int t = 0; t < s; ++t) v[t] += v[t + s];
    return v[0];
}

// ---- what both trainers keep ---------------------------------------------------------------------------------------------------
struct Model {
    int32_t orders[2][BT_K];
    std::vector<float> ps[2];  // [20][4][4096]
    float gc_qs[BT_GC_BINS - 1];
    float gc_bins[BT_GC_EXPANDED];
    double accuracy = 0.0;
    SearchState trace[2];
    bool trained = false;
};

struct Inputs {  // the arguments of polee_bias_train_create, borrowed for the call
    int32_t n;
    const int64_t *tseq_ptr;
    const uint8_t *tseq;
    int64_t n_fg;
    const int32_t *fg_t;
    const int64_t *fg_tpos;
    const int32_t *fg_fl;
    int64_t n_bg;
    const int32_t *bg_t;  // null: drawn
    const int64_t *bg_tpos;
    const int32_t *bg_fl;
};
polee_status check_counts(polee_ctx *ctx, const char *who, int64_t n_fg, int64_t n_bg);
polee_status check_inputs(polee_ctx *ctx, const char *who, const Inputs &in);

// The host trainer (bias_train_host.cpp): what `host = 1` runs, over POLEE_HOST_THREADS.
class HostTrainer {
public:
    int64_t n_fg = 0, n_bg = 0;
    uint64_t seed = 0;
    std::vector<uint64_t> seq[2];  // [N], foreground first
    std::vector<double> gc;        // [N]
    std::vector<int64_t> bg_pos;   // [n_bg]: the positions of the background fragments (drawn or given); empty from examples
    Model model;

    void from_fragments(const Inputs &in, uint64_t seed_);
    void from_examples(int64_t n_fg_, int64_t n_bg_, const uint8_t *left, const uint8_t *right, const double *frag_gc);
    void run();
    void candidates(int side, const int32_t *orders_in, double *losses_out, double *loss0_out);

private:
    int64_t N() const { return n_fg + n_bg; }
    SearchState st;
    std::vector<uint32_t> cnt;          // [20][BT_TABLE] counts of every position's candidate
    std::vector<float> cand, cur, fac;  // [20][BT_TABLE] tables; fac [2][20][N]
    void reset_side();
    void count_table(int side, int j, int o);
    void commit(int side, int j);
    void losses(int side, double *sums);
    void finish_side(int side);
    void gc_and_accuracy();
};

}  // namespace biastrain
}  // namespace polee

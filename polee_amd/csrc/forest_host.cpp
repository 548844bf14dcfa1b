// The forest of `polee model random-forest` on the host: the definition of forest_common.hpp built tree by
// tree, trees in parallel over POLEE_HOST_THREADS.  It is what `--host` runs, and the tests hold the device builder (forest.hip)
// against it node for node.  Free functions over caller arrays; no context, no device.
#include "common.hpp"
#include "forest_common.hpp"

#include <algorithm>
#include <cstring>

namespace polee {
namespace forest {

const char *check_opts(const polee_forest_opts &o, int32_t n, int32_t k)
{
    if (n < 1) return "n < 1";
    if (k < 2 || k > FO_MAX_K) return "the number of classes must be 2..16";
    if (o.ntrees < 1 || o.ntrees > FO_MAX_TREES) return "ntrees must be 1..65536";
    if (o.max_depth < -1) return "max_depth must be -1 (no limit) or at least 0";
    if (o.min_samples_leaf < 1 || o.min_samples_split < 1) return "min_samples_leaf and min_samples_split must be at least 1";
    if (!(o.nsubfeatures > 0.0) || !std::isfinite(o.nsubfeatures)) return "nsubfeatures must be positive";
    if (!(o.partial_sampling > 0.0) || !std::isfinite(o.partial_sampling)) return "partial_sampling must be positive";
    return nullptr;
}

bool nodes_ok(int32_t n, int32_t k, int32_t ntrees, const int64_t *tree_off, const int32_t *feature, const int32_t *left,
              const int32_t *right, const int32_t *label, int32_t *bad_tree, int64_t *bad_node)
{
    for (int32_t t = 0; t < ntrees; ++t) {
        const int64_t b = tree_off[t], cnt = tree_off[t + 1] - b;
        *bad_tree = t;
        *bad_node = -1;
        if ((t == 0 && b != 0) || cnt < 1 || cnt > INT32_MAX) return false;
        for (int64_t i = 0; i < cnt; ++i) {
            const int32_t f = feature[b + i], l = left[b + i], r = right[b + i];
            *bad_node = i;
            if (f < -1 || f >= n || label[b + i] < 0 || label[b + i] >= k) return false;
            if (f >= 0 && (l <= i || l >= cnt || r <= i || r >= cnt)) return false;
        }
    }
    return true;
}

namespace {

struct Tree {
    std::vector<int32_t> feature, left, right, label;
    std::vector<double> threshold;
};

void build_tree(const float *x, const int32_t *labels, int32_t N, int32_t n, int32_t k, const polee_forest_opts &o, int32_t nsub,
                int32_t Nb, uint64_t seed, uint32_t t, const double *T, Tree &out)
{
    struct Seg {
        int32_t beg, end, depth;
    };
    std::vector<int32_t> rows((size_t)Nb);
    for (int32_t i = 0; i < Nb; ++i) rows[(size_t)i] = (int32_t)boot_row(seed, t, (uint32_t)i, (uint32_t)N);
    std::vector<Seg> segs{{0, Nb, 0}};
    std::vector<uint64_t> keys;
    auto push_node = [&]() {
        out.feature.push_back(-1);
        out.left.push_back(-1);
        out.right.push_back(-1);
        out.label.push_back(0);
        out.threshold.push_back(0.0);
    };
    push_node();
    // (children are appended as their parent is met, so the numbering is level by level, parents' order, left before right)
    for (size_t node = 0; node < segs.size(); ++node) {
        const Seg sg = segs[node];
        const int32_t cnt = sg.end - sg.beg;
        int32_t tot[FO_MAX_K] = {0};
        for (int32_t i = sg.beg; i < sg.end; ++i) ++tot[labels[rows[(size_t)i]]];
        int32_t best_c = 0;
        for (int c = 1; c < k; ++c)
            if (tot[c] > tot[best_c]) best_c = c;
        out.label[node] = best_c;
        if (tot[best_c] == cnt || cnt < o.min_samples_split || sg.depth == o.max_depth) continue;
        bool found = false;
        double best_score = 0.0, best_thr = 0.0;
        int32_t best_f = -1;
        keys.resize((size_t)cnt);
        for (int32_t pos = 0; pos < nsub; ++pos) {
            const uint32_t f = candidate_feature(seed, t, (uint32_t)node, (uint32_t)n, (uint32_t)pos);
            for (int32_t i = 0; i < cnt; ++i) {
                const int32_t r = rows[(size_t)(sg.beg + i)];
                uint32_t u;
                std::memcpy(&u, &x[(size_t)r * n + f], 4);
                keys[(size_t)i] = ((uint64_t)sortable_bits(u) << 32) | (uint32_t)labels[r];
            }
            if ((keys[0] >> 32) == (keys[(size_t)cnt - 1] >> 32) && std::all_of(keys.begin(), keys.end(), [&](uint64_t q) {
                    return (q >> 32) == (keys[0] >> 32);
                }))
                continue;  // (a constant candidate has no boundary)
            std::sort(keys.begin(), keys.end());
            int32_t cl[FO_MAX_K] = {0};
            for (int32_t i = 1; i < cnt; ++i) {
                ++cl[(uint32_t)keys[(size_t)i - 1]];
                if (i < o.min_samples_leaf || cnt - i < o.min_samples_leaf) continue;
                const uint32_t ua = unsortable_bits((uint32_t)(keys[(size_t)i - 1] >> 32)), ub = unsortable_bits((uint32_t)(keys[(size_t)i] >> 32));
                float lo, hi;
                std::memcpy(&lo, &ua, 4);
                std::memcpy(&hi, &ub, 4);
                if (!(lo < hi)) continue;
                const double s = boundary_score(T, cl, tot, k, i, cnt - i);
                if (!found || s > best_score) {  // (ties: the earlier position, then the earlier boundary = the smaller threshold)
                    found = true;
                    best_score = s;
                    best_thr = threshold_of(lo, hi);
                    best_f = (int32_t)f;
                }
            }
        }
        if (!found) continue;
        const auto mid = std::stable_partition(rows.begin() + sg.beg, rows.begin() + sg.end,
                                               [&](int32_t r) { return (double)x[(size_t)r * n + best_f] < best_thr; });
        const int32_t m = (int32_t)(mid - rows.begin());
        out.feature[node] = best_f;
        out.threshold[node] = best_thr;
        out.left[node] = (int32_t)segs.size();
        out.right[node] = (int32_t)segs.size() + 1;
        segs.push_back({sg.beg, m, sg.depth + 1});
        segs.push_back({m, sg.end, sg.depth + 1});
        push_node();
        push_node();
    }
}

}  // namespace
}  // namespace forest
}  // namespace polee

using namespace polee;
using namespace polee::forest;

extern "C" {

void polee_forest_default_opts(polee_forest_opts *o)
{
    if (!o) return;
    o->ntrees = 200;
    o->max_depth = -1;
    o->min_samples_leaf = 1;
    o->min_samples_split = 2;
    o->nsubfeatures = 10.0;
    o->partial_sampling = 1.0;
}

polee_status polee_forest_build_host(const float *x, const int32_t *labels, int32_t N, int32_t n, int32_t k,
                                     const polee_forest_opts *opts, uint64_t seed, int64_t capacity, int64_t *nnodes, int64_t *tree_off,
                                     int32_t *feature, double *threshold, int32_t *left, int32_t *right, int32_t *label)
{
    return host_entry("polee_forest_build_host", [&]() -> polee_status {
        if (!x || !labels || !nnodes || N < 1) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_forest_build_host: bad argument");
        polee_forest_opts o;
        polee_forest_default_opts(&o);
        if (opts) o = *opts;
        if (const char *why = check_opts(o, n, k)) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_forest_build_host: %s", why);
        const int64_t Nb64 = nboot_of(N, o.partial_sampling);
        if (Nb64 > POLEE_FOREST_MAX_ROWS)
            return fail(nullptr, POLEE_ERR_UNSUPPORTED, "polee_forest_build_host: %lld rows per tree; the builders take up to %d",
                        (long long)Nb64, POLEE_FOREST_MAX_ROWS);
        for (int32_t i = 0; i < N; ++i)
            if (labels[i] < 0 || labels[i] >= k) return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_forest_build_host: label %d of row %d", labels[i], i);
        const size_t Nn = (size_t)N * n;
        for (size_t i = 0; i < Nn; ++i)
            if (!std::isfinite(x[i]))
                return fail(nullptr, POLEE_ERR_NONFINITE,
                            "polee_forest_build_host: x[%zu][%zu] is not finite (log of a zero point estimate? add a pseudocount)", i / n,
                            i % n);
        const int32_t Nb = (int32_t)Nb64, nsub = nsub_of(n, o.nsubfeatures);
        std::vector<double> T((size_t)Nb + 1);
        clogc_table(T.data(), Nb);
        std::vector<Tree> trees((size_t)o.ntrees);
        parallel_chunks((size_t)o.ntrees, 1, [&](size_t lo, size_t hi, unsigned) {
            for (size_t t = lo; t < hi; ++t) build_tree(x, labels, N, n, k, o, nsub, Nb, seed, (uint32_t)t, T.data(), trees[t]);
        });
        int64_t total = 0;
        for (const Tree &tr : trees) total += (int64_t)tr.feature.size();
        *nnodes = total;
        if (!feature && !threshold && !left && !right && !label && !tree_off) return POLEE_OK;
        if (!feature || !threshold || !left || !right || !label || !tree_off)
            return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_forest_build_host: some node arrays are null");
        if (total > capacity)
            return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_forest_build_host: %lld nodes, room for %lld", (long long)total, (long long)capacity);
        int64_t at = 0;
        for (size_t t = 0; t < trees.size(); ++t) {
            const Tree &tr = trees[t];
            tree_off[t] = at;
            std::copy(tr.feature.begin(), tr.feature.end(), feature + at);
            std::copy(tr.threshold.begin(), tr.threshold.end(), threshold + at);
            std::copy(tr.left.begin(), tr.left.end(), left + at);
            std::copy(tr.right.begin(), tr.right.end(), right + at);
            std::copy(tr.label.begin(), tr.label.end(), label + at);
            at += (int64_t)tr.feature.size();
        }
        tree_off[trees.size()] = at;
        return POLEE_OK;
    });
}

polee_status polee_forest_votes_host(int32_t n, int32_t k, int32_t ntrees, const int64_t *tree_off, const int32_t *feature,
                                     const double *threshold, const int32_t *left, const int32_t *right, const int32_t *label,
                                     const float *x, int32_t R, int32_t *votes)
{
    return host_entry("polee_forest_votes_host", [&]() -> polee_status {
        if (!tree_off || !feature || !threshold || !left || !right || !label || !x || !votes || n < 1 || k < 1 || ntrees < 1 || R < 1)
            return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_forest_votes_host: bad argument");
        int32_t bt = 0;
        int64_t bn = 0;
        if (!nodes_ok(n, k, ntrees, tree_off, feature, left, right, label, &bt, &bn))
            return fail(nullptr, POLEE_ERR_BAD_ARG, "polee_forest_votes_host: node %lld of tree %d is malformed", (long long)bn, bt);
        std::fill(votes, votes + (size_t)R * k, 0);
        parallel_chunks((size_t)R, 64, [&](size_t lo, size_t hi, unsigned) {
            for (size_t r = lo; r < hi; ++r)
                for (int32_t t = 0; t < ntrees; ++t) {
                    const int64_t b = tree_off[t];
                    int32_t i = 0;
                    while (feature[b + i] >= 0) i = (double)x[r * n + feature[b + i]] < threshold[b + i] ? left[b + i] : right[b + i];
                    ++votes[r * k + label[b + i]];
                }
        });
        return POLEE_OK;
    });
}

}  // extern "C"

// Sanitizer driver for the host builder of `polee model random-forest` (polee_amd/csrc/forest_host.cpp): forests on planted-signal
// data of two shapes (few rows and many classes; more rows, constant and rounded columns, a partial bootstrap, a depth limit and a
// larger min_samples_leaf), the count-only call, a capacity that is too small, the votes of the forests on fresh rows, and the
// rejection of malformed input and malformed node arrays.  Built host-only (--offload-host-only) with
// -fsanitize=address,undefined by `make -C polee_amd/csrc sanitize-forest` and run there on the CPU; it touches no GPU and is not
// loaded into Python.  Exit code 0 = every call did what it should (the sanitizer itself aborts on a finding).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../include/polee_hip.h"

static int fails = 0;
#define REQUIRE(cond)                                                   \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__);  \
            ++fails;                                                    \
        }                                                               \
    } while (0)

struct Forest {
    std::vector<int64_t> off;
    std::vector<int32_t> feature, left, right, label;
    std::vector<double> threshold;
};

static void planted(std::mt19937_64 &rng, int32_t N, int32_t n, int32_t k, bool rounded, std::vector<float> &x, std::vector<int32_t> &y)
{
    std::normal_distribution<float> g(0.0f, 1.0f);
    x.resize((size_t)N * n);
    y.resize((size_t)N);
    for (int32_t i = 0; i < N; ++i) {
        y[(size_t)i] = (int32_t)(rng() % (uint64_t)k);
        for (int32_t j = 0; j < n; ++j) {
            float v = g(rng);
            if (j / 3 == y[(size_t)i]) v += 2.0f;
            if (j >= n - 4) v = 0.25f;  // constant columns
            if (rounded) v = std::round(v * 10.0f) / 10.0f;
            x[(size_t)i * n + j] = v;
        }
    }
}

static void build_and_vote(std::mt19937_64 &rng, int32_t N, int32_t n, int32_t k, polee_forest_opts o, bool rounded)
{
    std::vector<float> x, xt;
    std::vector<int32_t> y, yt;
    planted(rng, N, n, k, rounded, x, y);
    int64_t count = 0, count2 = 0;
    REQUIRE(polee_forest_build_host(x.data(), y.data(), N, n, k, &o, 7, 0, &count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
            POLEE_OK);
    REQUIRE(count >= o.ntrees);
    Forest f;
    f.off.resize((size_t)o.ntrees + 1);
    f.feature.resize((size_t)count);
    f.left.resize((size_t)count);
    f.right.resize((size_t)count);
    f.label.resize((size_t)count);
    f.threshold.resize((size_t)count);
    if (count > 1)
        REQUIRE(polee_forest_build_host(x.data(), y.data(), N, n, k, &o, 7, count - 1, &count2, f.off.data(), f.feature.data(),
                                        f.threshold.data(), f.left.data(), f.right.data(), f.label.data()) == POLEE_ERR_BAD_ARG);
    REQUIRE(polee_forest_build_host(x.data(), y.data(), N, n, k, &o, 7, count, &count2, f.off.data(), f.feature.data(), f.threshold.data(),
                                    f.left.data(), f.right.data(), f.label.data()) == POLEE_OK);
    REQUIRE(count2 == count && f.off[0] == 0 && f.off[(size_t)o.ntrees] == count);
    const int32_t R = 37;
    planted(rng, R, n, k, rounded, xt, yt);
    std::copy(x.begin(), x.begin() + n, xt.begin());  // (a row the forest has seen: values equal to thresholds' neighbours)
    std::vector<int32_t> votes((size_t)R * k);
    REQUIRE(polee_forest_votes_host(n, k, o.ntrees, f.off.data(), f.feature.data(), f.threshold.data(), f.left.data(), f.right.data(),
                                    f.label.data(), xt.data(), R, votes.data()) == POLEE_OK);
    int32_t hits = 0;
    for (int32_t r = 0; r < R; ++r) {
        int32_t sum = 0, best = 0;
        for (int32_t c = 0; c < k; ++c) {
            sum += votes[(size_t)r * k + c];
            if (votes[(size_t)r * k + c] > votes[(size_t)r * k + best]) best = c;
        }
        REQUIRE(sum == o.ntrees);
        hits += best == yt[(size_t)r] || r == 0;
    }
    if (o.max_depth < 0 && o.ntrees >= 7 && k <= 3) REQUIRE(hits > R / 2);  // (7 trees on 16 classes of 6 rows each learn little)
    // malformed node arrays: a child before its parent
    if (f.feature[0] >= 0) {
        Forest b = f;
        b.left[0] = 0;
        REQUIRE(polee_forest_votes_host(n, k, o.ntrees, b.off.data(), b.feature.data(), b.threshold.data(), b.left.data(), b.right.data(),
                                        b.label.data(), xt.data(), R, votes.data()) == POLEE_ERR_BAD_ARG);
    }
    // malformed input
    x[5] = std::numeric_limits<float>::infinity();
    REQUIRE(polee_forest_build_host(x.data(), y.data(), N, n, k, &o, 7, 0, &count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
            POLEE_ERR_NONFINITE);
    x[5] = 0.0f;
    y[0] = k;
    REQUIRE(polee_forest_build_host(x.data(), y.data(), N, n, k, &o, 7, 0, &count, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
            POLEE_ERR_BAD_ARG);
}

int main()
{
    std::mt19937_64 rng(5);
    polee_forest_opts o;
    polee_forest_default_opts(&o);
    REQUIRE(o.ntrees == 200 && o.max_depth == -1 && o.min_samples_leaf == 1 && o.min_samples_split == 2);
    o.ntrees = 7;
    o.nsubfeatures = 1.0;
    build_and_vote(rng, 96, 130, 16, o, false);
    o.partial_sampling = 0.7;
    o.min_samples_leaf = 3;
    build_and_vote(rng, 200, 1100, 3, o, true);
    o.max_depth = 1;
    o.ntrees = 1;
    build_and_vote(rng, 40, 150, 3, o, false);
    if (fails) return 1;
    printf("forest host builder: ok\n");
    return 0;
}

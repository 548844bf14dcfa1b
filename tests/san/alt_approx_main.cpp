// Sanitizer driver for the host parts of the alternative likelihood approximations (polee_amd/csrc/altvi_host.cpp): the
// reference's constants per method, and the ILR coefficient table on a caterpillar, a balanced and a two-leaf tree, checked against
// the identities a^2 r + b^2 s = 1 and a r + b s = 0 (the balance of a node is a unit vector orthogonal to the constant), plus the
// rejection of malformed input.  Built host-only (--offload-host-only) with -fsanitize=address,undefined by
// `make -C polee_amd/csrc sanitize-alt-approx` and run there on the CPU; it touches no GPU and is not loaded into Python.
// Exit code 0 = every call did what it should (the sanitizer itself aborts on a finding).
#include <cmath>
#include <cstdint>
#include <cstdio>
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

static void check_table(const std::vector<int32_t> &r, const std::vector<int32_t> &s)
{
    std::vector<double> ab(r.size() * 2, 0.0);
    REQUIRE(polee_ilr_coefficients(r.data(), s.data(), (int64_t)r.size(), ab.data()) == POLEE_OK);
    for (size_t k = 0; k < r.size(); ++k) {
        const double a = ab[2 * k], b = ab[2 * k + 1];
        REQUIRE(a > 0.0 && b < 0.0);
        REQUIRE(std::fabs(a * a * r[k] + b * b * s[k] - 1.0) < 1e-12);
        REQUIRE(std::fabs(a * r[k] + b * s[k]) < 1e-12);
    }
}

int main()
{
    // the constants of every method (likelihood-approximation-alt.jl:66-67, 225-226, 348-349, 520-521, 637-638)
    const int32_t methods[5] = {POLEE_ALT_LOGISTIC_NORMAL, POLEE_ALT_KUMARASWAMY_PTT, POLEE_ALT_LOGIT_NORMAL_PTT, POLEE_ALT_NORMAL_ILR,
                                POLEE_ALT_NORMAL_ALR};
    const double steps[5] = {2e-2, 1e-1, 2e-1, 2e-1, 2e-1};
    for (int i = 0; i < 5; ++i) {
        polee_altvi_opts o;
        polee_altvi_default_opts(methods[i], &o);
        REQUIRE(o.method == methods[i] && o.num_steps == 500 && o.num_mc_samples == 6 && o.gradonly == 1 && o.refidx == -1);
        REQUIRE(o.max_step0 == steps[i] && o.max_step1 == steps[i] && o.eps == 1e-10 && o.z0 == nullptr);
        REQUIRE(o.adam_rm == 0.7 && o.adam_rv == 0.9 && o.adam_eps == 1e-8);
    }
    polee_altvi_default_opts(POLEE_ALT_NORMAL_ILR, nullptr);  // (a null pointer is ignored)

    // a caterpillar of 2000 leaves: one child is a leaf, the other everything below
    {
        const int32_t n = 2000;
        std::vector<int32_t> r, s;
        for (int32_t k = 0; k + 1 < n; ++k) {
            r.push_back(k % 2 ? 1 : n - 1 - k);
            s.push_back(k % 2 ? n - 1 - k : 1);
        }
        check_table(r, s);
    }
    // a balanced tree of 1024 leaves, level by level
    {
        std::vector<int32_t> r, s;
        for (int32_t size = 1024; size >= 2; size /= 2)
            for (int32_t i = 0; i < 1024 / size; ++i) {
                r.push_back(size / 2);
                s.push_back(size / 2);
            }
        check_table(r, s);
    }
    check_table({1}, {1});  // n = 2
    check_table({}, {});    // nothing to do
    // the largest counts an int32 tree can hold do not overflow the products
    check_table({2147483646}, {1});
    // malformed input
    {
        std::vector<int32_t> r{1, 0}, s{1, 3};
        std::vector<double> ab(4);
        REQUIRE(polee_ilr_coefficients(r.data(), s.data(), 2, ab.data()) == POLEE_ERR_BAD_ARG);
        REQUIRE(polee_ilr_coefficients(nullptr, s.data(), 2, ab.data()) == POLEE_ERR_BAD_ARG);
        REQUIRE(polee_ilr_coefficients(r.data(), s.data(), -1, ab.data()) == POLEE_ERR_BAD_ARG);
        REQUIRE(polee_last_error(nullptr) != nullptr);
    }
    if (fails) {
        fprintf(stderr, "%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}

// Host parts of the alternative likelihood approximations (altvi.hip): the reference's constants per method and the ILR
// coefficient table.  Nothing here touches the device, so that the sanitizer driver
// tests/san/alt_approx_main.cpp can link this file with ctx.hip alone.
#include "common.hpp"

#include <cmath>

using polee::host_entry;

extern "C" {

void polee_altvi_default_opts(int32_t method, polee_altvi_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->method = method;
    o->num_steps = 500;      // LIKAP_NUM_STEPS (constants.jl:64)
    o->num_mc_samples = 6;   // LIKAP_NUM_MC_SAMPLES (constants.jl:65)
    o->gradonly = 1;
    o->refidx = -1;          // NormalALRApprox() = NormalALRApprox(-1): the last element (likelihood-approximation-alt.jl:47, 641)
    o->seed = 123456789ull;  // main.jl:126
    o->z0 = nullptr;
    o->eps = 1e-10;          // `eps = 1e-10` (likelihood-approximation-alt.jl:109, 562, 681)
    o->adam_initial_learning_rate = 1.0;
    o->adam_learning_rate_decay = 2e-2;
    o->adam_min_learning_rate = 1e-3;
    o->adam_eps = 1e-8;
    o->adam_rv = 0.9;
    o->adam_rm = 0.7;
    // ss_max_*_step (likelihood-approximation-alt.jl:66-67, 225-226, 348-349, 520-521, 637-638)
    const double ms = method == POLEE_ALT_LOGISTIC_NORMAL ? 2e-2 : method == POLEE_ALT_KUMARASWAMY_PTT ? 1e-1 : 2e-1;
    o->max_step0 = ms;
    o->max_step1 = ms;
}

// a = sqrt(s / (r (r + s))), b = -sqrt(r / (s (r + s))) with r, s the leaves below the left and the right child
// (isometric_log_ratios.jl:62-66); ab [count][2]
polee_status polee_ilr_coefficients(const int32_t *r, const int32_t *s, int64_t count, double *ab)
{
    return host_entry("polee_ilr_coefficients", [&]() -> polee_status {
        if (count < 0 || (count > 0 && (!r || !s || !ab))) return polee::fail(nullptr, POLEE_ERR_BAD_ARG, "polee_ilr_coefficients: bad argument");
        for (int64_t k = 0; k < count; ++k) {
            if (r[k] < 1 || s[k] < 1)
                return polee::fail(nullptr, POLEE_ERR_BAD_ARG, "polee_ilr_coefficients: node %lld has %d and %d leaves below its children", (long long)k,
                                   r[k], s[k]);
            const double rr = (double)r[k], ss = (double)s[k];
            ab[2 * k + 0] = std::sqrt(ss / (rr * (rr + ss)));
            ab[2 * k + 1] = -std::sqrt(rr / (ss * (rr + ss)));
        }
        return POLEE_OK;
    });
}

}  // extern "C"

// The ADAM constants of one step, shared by the VI fit (vi.hip) and the alternative approximations (altvi.hip).
#pragma once
#include <algorithm>
#include <cmath>

namespace polee {

struct AdamConsts {
    double lr, rm, rv, eps, m_denom, v_denom;
    double inv_m_denom, inv_v_denom;  // reciprocals, computed once on the host (the update kernel is bound by its f64 instructions)
    double max_mu, max_omega, max_alpha;
    int first;  // step_num == 1
};

// The schedule of step `step_num` (1-based) from the options of either fit (polee_vi_opts, polee_altvi_opts): the decayed learning
// rate, adam_learning_rate(step_num - 1) (likelihood-approximation.jl:107-110, 497), and the bias corrections.  The step caps are
// the caller's.
template <class Opts>
inline AdamConsts adam_schedule(const Opts &o, int step_num)
{
    AdamConsts a;
    a.lr = std::max(o.adam_min_learning_rate,
                    o.adam_initial_learning_rate * std::exp(-o.adam_learning_rate_decay * (double)(step_num - 1)));
    a.rm = o.adam_rm;
    a.rv = o.adam_rv;
    a.eps = o.adam_eps;
    a.m_denom = 1 - std::pow(o.adam_rm, (double)step_num);
    a.v_denom = 1 - std::pow(o.adam_rv, (double)step_num);
    a.inv_m_denom = 1.0 / a.m_denom;
    a.inv_v_denom = 1.0 / a.v_denom;
    a.max_mu = a.max_omega = a.max_alpha = 0.0;
    a.first = step_num == 1;
    return a;
}

}  // namespace polee

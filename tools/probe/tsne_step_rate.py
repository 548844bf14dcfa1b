"""Step rate of `polee model tsne`: RNASeqTSNE.fit's device loop.

    python tools/probe/tsne_step_rate.py [--reps 5] [--steps 40] [--out profiles/tsne_step_rate.txt]

S = 64 samples, n = 200 000 transcripts, C = 2 components, B = 64, synthetic approximations on one shared tree as
`bench.py --workload c3` makes them.  Every repetition times one polee_tsne_fit call of --steps steps (host clock around the call,
which returns after the last step has run; a warm-up call first) and, for comparison, the same number of bare sampler draws
(RNASeqApproxLikelihood.sample, download included).  Prints steps/s and microseconds per step, median [min .. max].  The share of
each kernel comes from a kernel trace of a run of this script (rocprofv3 --kernel-trace --stats -- python tools/probe/tsne_step_rate.py
--reps 1), not from this script.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S, N, C, B = 64, 200000, 2, 64


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out")
    a = ap.parse_args()
    import polee_amd as P
    from polee_amd import tsne
    from tools import synth
    ctx = P.Context(0)
    rng = np.random.default_rng(0)
    smp = synth.make_sample(N, 1000000, 8.0, 1)
    parents, js = synth.make_tree(smp["gene"], 1)
    li, ri, fi = P.make_inverse_ptt_params(parents, js)
    lik = P.RNASeqApproxLikelihood(dict(efflen=np.tile(smp["effective_lengths"], (S, 1)).astype(np.float32),
                                        la_mu=rng.normal(0, 2, (S, N - 1)).astype(np.float32),
                                        la_sigma=np.exp(rng.normal(-1, 1, (S, N - 1))).astype(np.float32),
                                        la_alpha=rng.normal(0, .3, (S, N - 1)).astype(np.float32), left_index=li[None],
                                        right_index=ri[None], leaf_index=fi[None]), ctx=ctx)
    ts = P.RNASeqTSNE(N, S, ctx=ctx, num_components=C)
    t0 = time.perf_counter()
    ts.find_sigmas(lik, seed=1)
    t_sigmas = time.perf_counter() - t0
    ts.set_params(tsne.initial_weights(1, N, C))
    trace = ts.fit(5, lik, batch_size=B, seed=2)  # warm-up
    rates = []
    for r in range(a.reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        trace = ts.fit(a.steps, lik, batch_size=B, seed=3 + r)
        rates.append(a.steps / (time.perf_counter() - t0))
    draws = []
    for r in range(a.reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(3):
            lik.sample(seed=50 + i)
        draws.append((time.perf_counter() - t0) / 3)
    us = [1e6 / v for v in rates]
    lines = ["tsne_step_rate: S = %d, n = %d, C = %d, B = %d, %d steps per timing, %d repetitions" % (S, N, C, B, a.steps, a.reps),
             "build: " + P.version(),
             "  steps/s                         %9.1f  [%9.1f .. %9.1f]" % (np.median(rates), min(rates), max(rates)),
             "  us per step                     %9.1f  [%9.1f .. %9.1f]" % (np.median(us), min(us), max(us)),
             "  us per bare sampler draw + download of x (for scale)  %9.1f" % (1e6 * np.median(draws)),
             "  find_sigmas (one draw, the S x S distances, 20 bisection steps per row on the host): %.3f s" % t_sigmas,
             "  loss trace finite: %s, last loss %.6g" % (bool(np.all(np.isfinite(trace))), trace[-1])]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

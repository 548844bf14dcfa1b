"""Step rate of `polee model classify`: RNASeqLogisticRegression.fit_sample's device loop at the reference's defaults.

    python tools/probe/classify_step_rate.py [--reps 5] [--steps 40] [--out profiles/classify_step_rate.txt]

S = 64 samples, n = 200 000 transcripts, k = 4 classes, 5 draws per step, synthetic approximations on one shared tree as
`bench.py --workload c3` makes them.  Every repetition times one polee_classify_fit call of --steps steps (host clock around the call,
which returns after the last step has run; a warm-up call first) and, for comparison, the same number of bare sampler draws
(RNASeqApproxLikelihood.sample, download included).  Prints steps/s and microseconds per draw, median [min .. max].
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S, N, K, D = 64, 200000, 4, 5


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out")
    a = ap.parse_args()
    import polee_amd as P
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
    y = np.eye(K, dtype=np.float32)[np.arange(S) % K]
    clf = P.RNASeqLogisticRegression(K, N, ctx=ctx, draws_per_step=D)
    clf.init_bias_sample(S, N, lik, seed=1)
    trace = clf.fit_steps_sample(S, N, lik, y, 5, seed=2)  # warm-up
    rates = []
    for r in range(a.reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        trace = clf.fit_steps_sample(S, N, lik, y, a.steps, seed=3 + r)
        rates.append(a.steps / (time.perf_counter() - t0))
    draws = []
    for r in range(a.reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(3):
            lik.sample(seed=50 + i)
        draws.append((time.perf_counter() - t0) / 3)
    us = [1e6 / (v * D) for v in rates]
    lines = ["classify_step_rate: S = %d, n = %d, k = %d, %d draws per step, %d steps per timing, %d repetitions" % (S, N, K, D, a.steps,
                                                                                                                  a.reps),
             "build: " + P.version(),
             "  steps/s                         %9.1f  [%9.1f .. %9.1f]" % (np.median(rates), min(rates), max(rates)),
             "  us per draw (whole step / %d)    %9.1f  [%9.1f .. %9.1f]" % (D, np.median(us), min(us), max(us)),
             "  us per bare sampler draw + download of x (for scale)  %9.1f" % (1e6 * np.median(draws)),
             "  loss trace finite: %s, last loss %.6g" % (bool(np.all(np.isfinite(trace))), trace[-1])]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

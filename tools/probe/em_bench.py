"""EM (csrc/em.hip) cost per iteration: HIP-event time over EM_BENCH_ITERS (default 200) queued iterations at C2 (literal
generator) and on the real fixture tiled x639; the noise floor of the pass's lp at a fixed mixture (20
evaluations with float atomics; on the fixture also the gap to an f64 NumPy evaluation); wall time and iteration count of a run
with the reference's defaults (tol 1e-6) at C2; the wall time of the f64 fixed-point residual.  Output: one line per measurement on stdout.
EM_BENCH_QUICK=c2 | fixture: the timed iterations on that input only -- the profiler runs: `rocprofv3 --kernel-trace --stats` for the per-kernel medians, `rocprofv3 --hip-trace --stats` for the stream
synchronisations per run (10 warm-up iterations in one polee_em_run, then three runs of EM_BENCH_ITERS)."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import polee_amd as P  # noqa: E402
from polee_amd.em import EM  # noqa: E402
from tools import synth  # noqa: E402

N, M = 200_000, 30_000_000
ITERS = int(os.environ.get("EM_BENCH_ITERS", "200"))
CHECK_EVERY = int(os.environ.get("EM_BENCH_CHECK_EVERY", "64"))
QUICK = os.environ.get("EM_BENCH_QUICK", "")


def sample_of(ctx, smp):
    return P.RNASeqSample(smp["m"], smp["n"], None, None, None, smp["effective_lengths"], ctx=ctx,
                          xt=(smp["tcolptr"], smp["trowval"], smp["tnzval"]))


def timed_iterations(name, ctx, s):
    em = EM(s)
    em.run(10, -1.0, 10)
    best = None
    for _ in range(3):
        ctx.timer_start()
        em.run(ITERS, -1.0, CHECK_EVERY)
        ms = ctx.timer_stop() / (ITERS + 1)  # (+ 1: the pass behind the last update, for its lp)
        best = ms if best is None else min(best, ms)
    info = em.info()
    print("%-13s %8.2f us/iteration over %d iterations (best of 3; check_every %d)  M = %d  lp %.3f"
          % (name, 1e3 * best, ITERS, CHECK_EVERY, info["M"], info["last_lp"]), flush=True)
    return em


def lp_noise(name, s, y, lp64=None):
    lps = np.array([s.log_likelihood(y)[0] for _ in range(20)])
    line = "%-13s lp of the pass at a fixed mixture, 20 evaluations with float atomics: mean %.6f, max - min %.3g (%.3g of |lp|)" % (
        name, lps.mean(), lps.max() - lps.min(), (lps.max() - lps.min()) / abs(lps.mean()))
    if lp64 is not None:
        line += "; mean - f64 NumPy %.3g (%.3g of |lp|)" % (lps.mean() - lp64, abs(lps.mean() - lp64) / abs(lp64))
    print(line, flush=True)


def residual_time(name, ctx, em):
    em.info(kkt=True)
    ctx.synchronize()
    t0 = time.time()
    k = em.info(kkt=True)["kkt_max"]
    print("%-13s fixed-point residual on request (an f64 gradient over the layout): %.2f ms wall, kkt_max %.4g"
          % (name, 1e3 * (time.time() - t0), k), flush=True)


def reference_defaults(name, ctx, s):
    em = EM(s)
    ctx.synchronize()
    t0 = time.time()
    info = em.run(5000, 1e-6, 64)
    dt = time.time() - t0
    print("%-13s reference defaults (tol 1e-6, at most 5 000 iterations): %d iterations, %s, %.3f s wall, lp %.3f, last increase %.3g"
          % (name, info["iters"], "converged" if info["converged"] else "not converged", dt, info["last_lp"], info["last_increase"]),
          flush=True)


def main():
    ctx = P.Context(0)
    if QUICK != "fixture":
        lit = synth.make_sample(N, M, 8.0, seed=123456789, literal=True)
        s = sample_of(ctx, lit)
        em = timed_iterations("c2-literal", ctx, s)
        if not QUICK:
            lp_noise("c2-literal", s, em.mixture())
            residual_time("c2-literal", ctx, em)
            reference_defaults("c2-literal", ctx, s)
        del em, s, lit
    if QUICK != "c2":
        s = sample_of(ctx, synth.tile_fixture(639))
        em = timed_iterations("fixture-x639", ctx, s)
        if not QUICK:
            lp_noise("fixture-x639", s, em.mixture())
            residual_time("fixture-x639", ctx, em)
            reference_defaults("fixture-x639", ctx, s)
            from test_em_host import Problem
            a = np.load(os.path.join(ROOT, "tests", "golden", "mBr_M_6w_1.likelihood-matrix.npz"))
            lm = dict(m=int(a["m"][0]), n=int(a["n"][0]), colptr=a["colptr"], rowval=a["rowval"], nzval=a["nzval"])
            s1 = P.RNASeqSample(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"], a["effective_lengths"], ctx=ctx)
            em1 = EM(s1)
            em1.run(200, -1.0)
            y = em1.mixture()
            lp_noise("fixture", s1, y, Problem.from_csc(lm).lp64(y.astype(np.float64)))


if __name__ == "__main__":
    main()

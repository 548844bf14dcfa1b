"""`polee sample` throughput at C2's size (n = 200 000 transcripts, m = 30 M reads, a seeded synthetic fit): ms per draw, SAMPLE_PROBE_DRAWS
(default 1000) draws in batches of SAMPLE_PROBE_BATCH (default 16), for
  - the raw draw alone (polee_sampler_draw: what was there before the streaming handle), and the same followed by the NumPy
    post-processing a user had to write (divide by the effective lengths, renormalise, expected counts, running mean),
  - the handle with props only, with expected counts, and with sampled counts at m = 3 M, 30 M and 300 M.
Every timing ends with a device synchronise (the downloads of a call wait for the stream) and follows a warm-up of one batch;
each point is timed over SAMPLE_PROBE_REPS (default 5) windows, median, minimum and maximum shown.
Output: one line per measurement on stdout (profiles/sample_throughput.txt)."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import polee_amd as P  # noqa: E402
from conftest import random_tree  # noqa: E402
from polee_amd.sample import ApproxSampleStream  # noqa: E402

N = int(os.environ.get("SAMPLE_PROBE_N", "200000"))
DRAWS = int(os.environ.get("SAMPLE_PROBE_DRAWS", "1000"))
BATCH = int(os.environ.get("SAMPLE_PROBE_BATCH", "16"))
REPS = int(os.environ.get("SAMPLE_PROBE_REPS", "5"))
SEED = 123456789


def timed(name, warm, step, ctx):
    warm()
    ctx.synchronize()
    ms = []
    for _ in range(REPS):  # (a window of 1000 draws is a tenth of a second: repeated, and the spread shown)
        t0 = time.perf_counter()
        done = 0
        while done < DRAWS:
            k = min(BATCH, DRAWS - done)
            step(k)
            done += k
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / DRAWS)
    print("%-58s median %7.3f ms/draw  (min %.3f, max %.3f over %d windows of %d draws in batches of %d)"
          % (name, float(np.median(ms)), min(ms), max(ms), REPS, DRAWS, BATCH), flush=True)
    return float(np.median(ms))


def main():
    rng = np.random.default_rng(SEED)
    parents, js = random_tree(N, rng, "balanced")
    ctx = P.Context(0)
    t = P.PolyaTreeTransform(parents, js, ctx=ctx)
    mu = rng.normal(0.0, 1.0, N - 1).astype(np.float32)
    sigma = np.exp(rng.normal(-2.0, 0.5, N - 1)).astype(np.float32)
    alpha = rng.normal(0.0, 0.1, N - 1).astype(np.float32)
    l = rng.uniform(200.0, 3000.0, N).astype(np.float32)
    print("n = %d, synthetic fit (balanced tree), seed %d; %s" % (N, SEED, P.version()), flush=True)

    als = P.ApproxLikelihoodSampler()
    als.set_transform(t, mu, sigma, alpha)
    als.seed(SEED)
    timed("raw draw alone (polee_sampler_draw)", lambda: als.rand(BATCH), lambda k: als.rand(k), ctx)

    m = 30_000_000
    acc = np.zeros(N, np.float64)
    l64 = l.astype(np.float64)

    def numpy_post(k):
        raw = als.rand(k)
        tt = raw / l[None, :]
        props = (tt.astype(np.float64) / tt.astype(np.float64).sum(axis=1)[:, None]).astype(np.float32)
        acc[:] += props.astype(np.float64).sum(axis=0)
        e = props.astype(np.float64) * l64[None, :]
        return e / e.sum(axis=1)[:, None] * m
    timed("raw draw + NumPy props, expected counts, running mean", lambda: numpy_post(BATCH), numpy_post, ctx)

    s = ApproxSampleStream(t, mu, sigma, alpha, l, m, SEED)
    timed("handle, props only", lambda: s.next(BATCH), lambda k: s.next(k), ctx)
    timed("handle, no output (posterior mean only)", lambda: s.next(BATCH, props=False), lambda k: s.next(k, props=False), ctx)
    timed("handle, expected counts", lambda: s.next(BATCH, props=False, counts=True), lambda k: s.next(k, props=False, counts=True), ctx)
    del s
    for mm in (3_000_000, 30_000_000, 300_000_000):
        s = ApproxSampleStream(t, mu, sigma, alpha, l, mm, SEED)
        timed("handle, sampled counts, m = %d" % mm, lambda: s.next(BATCH, props=False, counts=True, sample_counts=True),
              lambda k: s.next(k, props=False, counts=True, sample_counts=True), ctx)
        del s


if __name__ == "__main__":
    main()

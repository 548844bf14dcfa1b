"""Isoform effect sizes (csrc/effects.hip, polee_effects_run) at the size of C3: n = 200 000 transcripts in G ~ n / 3.4 genes whose
isoform counts follow SURVEY.md 8(d) (1 + Geometric(1 / 3.4) truncated to [1, 30]), F = 2 factors, niter = 1000 draws.  Prints the
kernel's HIP-event time (best and median of EFFECTS_BENCH_REPS runs after one warm-up, device noise), the wall time of a whole run
(uploads, kernel, downloads), and next to it the wall time of the NumPy restatement of the reference's loop
(tests/isoform_effects_restatement.py) on the first EFFECTS_BENCH_REF_GENES genes, scaled to all transcripts.  EFFECTS_BENCH_BIG=K
appends one gene of K isoforms (the path of genes with hundreds of isoforms is the same kernel).  One line per measurement on stdout."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import polee_amd as P  # noqa: E402
from polee_amd.regression import IsoformEffects  # noqa: E402

N = int(os.environ.get("EFFECTS_BENCH_N", "200000"))
F = int(os.environ.get("EFFECTS_BENCH_F", "2"))
NITER = int(os.environ.get("EFFECTS_BENCH_NITER", "1000"))
REPS = int(os.environ.get("EFFECTS_BENCH_REPS", "5"))
REF_GENES = int(os.environ.get("EFFECTS_BENCH_REF_GENES", "60"))
BIG = int(os.environ.get("EFFECTS_BENCH_BIG", "0"))


def gene_sizes(n, rng):
    sizes = []
    total = 0
    while total < n:
        k = min(int(rng.geometric(1.0 / 3.4)), 30)
        k = min(k, n - total)
        sizes.append(k)
        total += k
    return np.array(sizes)


def main():
    rng = np.random.default_rng(123456789)
    sizes = gene_sizes(N, rng)
    if BIG:
        sizes = np.append(sizes, BIG)
    n, G = int(sizes.sum()), sizes.size
    gene_sorted = np.repeat(np.arange(G), sizes)
    perm = rng.permutation(n)
    gene_of = np.empty(n, np.int32)
    gene_of[perm] = gene_sorted  # (the transcripts of a gene are scattered)
    qw_loc = rng.normal(0, 1, size=(F, n)).astype(np.float32)
    qw_scale = np.exp(rng.normal(-1.5, 0.7, size=(F, n))).astype(np.float32)
    bias_loc = rng.normal(-2, 3, size=n).astype(np.float32)
    bias_scale = np.exp(rng.normal(-1.5, 0.7, size=n)).astype(np.float32)
    ctx = P.Context(0)
    t0 = time.time()
    fx = IsoformEffects(gene_of, G, F, ctx=ctx)
    print("n = %d, G = %d (largest gene %d, single-isoform genes %d), F = %d, niter = %d; create %.1f ms wall"
          % (n, G, sizes.max(), int((sizes == 1).sum()), F, NITER, 1e3 * (time.time() - t0)), flush=True)
    kw = dict(niter=NITER, target_coverage=0.1, effect_size=float(np.log(1.5)), aitchison_effect_size=1.0, seed=123456789)
    first = fx.run(qw_loc, qw_scale, bias_loc, bias_scale, **kw)
    ms, wall, same = [], [], True
    for _ in range(REPS):
        t0 = time.time()
        out = fx.run(qw_loc, qw_scale, bias_loc, bias_scale, **kw)
        wall.append(1e3 * (time.time() - t0))
        ms.append(fx.kernel_ms)
        same = same and all(np.array_equal(a, b) for a, b in zip(first, out))  # (every repetition against the warm-up run)
    print("polee_effects_run kernel (HIP events): best %.3f ms, median %.3f ms of %d runs; whole call %.1f ms wall (median); all runs and the warm-up bitwise equal: %s"
          % (min(ms), float(np.median(ms)), REPS, float(np.median(wall)), same), flush=True)
    print("finite: %s; mean |mean effect| %.4f; mean Aitchison distance %.4f" % (all(np.isfinite(o).all() for o in out),
                                                                               float(np.abs(out[1]).mean()), float(out[4].mean())), flush=True)
    if REF_GENES > 0:
        import isoform_effects_restatement as T
        sub = np.nonzero(gene_of < REF_GENES)[0]
        zx = rng.normal(size=(NITER, sub.size))
        zw = rng.normal(size=(NITER, F, sub.size))
        t0 = time.time()
        T.estimate_isoform_effect_sizes(gene_of[sub], REF_GENES, kw["effect_size"], 1.0, qw_loc[:, sub], qw_scale[:, sub], bias_loc[sub],
                                        bias_scale[sub], zx, zw)
        dt = time.time() - t0
        print("NumPy restatement (one host thread, noise not counted): %.2f s for %d genes / %d transcripts -> %.0f s scaled to %d transcripts"
              % (dt, REF_GENES, sub.size, dt * n / sub.size, n), flush=True)


if __name__ == "__main__":
    main()

"""Step rate of the latent-design mode against the plain regression step, one box, interleaved repetitions.

    python tools/probe/pca_step_rate.py [--reps 7] [--out profiles/pca_step_rate.txt] [--parent-lib path/to/libpolee_hip.so]

n = 200 000 transcripts, C = 2 components, S = 6 and S = 64 samples, synthetic approximations as `bench.py --workload c3` makes them.
Configurations, timed in turn inside every repetition (fit of K steps on the device RNG = graph replays; warm-up fits excluded):
  (a) the plain regression step, F = 2;
  (c) the latent step: reg_design_grad_kernel for d(-log p)/dz + reg_latent_kernel (prior, Adam, clears the copies).
--parent-lib: (a) also from another build of the library (the parent commit's), in processes of their own run before and after this
build's repetitions.  Also the wall time of one 12 000-step RNASeqPCA.fit at S = 6.  Reports medians.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, C_DIM = 200000, 2
STEPS = {6: 300, 64: 60}


def inputs(P, ctx, S, seed=0):
    from tools import synth
    rng = np.random.default_rng(seed)
    smp = synth.make_sample(N, 1000000, 8.0, 1)
    parents, js = synth.make_tree(smp["gene"], 1)
    li, ri, fi = P.make_inverse_ptt_params(parents, js)
    vars_ = dict(efflen=np.tile(smp["effective_lengths"], (S, 1)).astype(np.float32),
                 la_mu=rng.normal(0, 2, (S, N - 1)).astype(np.float32),
                 la_sigma=np.exp(rng.normal(-1, 1, (S, N - 1))).astype(np.float32),
                 la_alpha=rng.normal(0, .3, (S, N - 1)).astype(np.float32), left_index=li[None], right_index=ri[None],
                 leaf_index=fi[None])
    x0 = np.empty((S, N), np.float32)
    for s0 in range(0, S, 8):
        sl = slice(s0, min(S, s0 + 8))
        v = {k: (a[sl] if a.shape[0] == S and S > 1 else a) for k, a in vars_.items()}
        x0[sl] = np.log(np.maximum(P.RNASeqApproxLikelihood(v, ctx=ctx).sample(seed=1 + s0), 1e-12))
    design = np.zeros((S, C_DIM), np.float32)
    design[:, 0] = 1
    design[S // 2:, 1] = 1
    return vars_, x0, design, P.estimate_sample_scales(x0, upper_quantile=0.9)


def timed(ctx, reg, steps):
    ctx.synchronize()
    t0 = time.perf_counter()
    reg._fit_steps(steps, 11)  # (synchronises before returning)
    return steps / (time.perf_counter() - t0)


def run(sizes, reps, only_a):
    import polee_amd as P
    ctx = P.Context(0)
    out = {"build": P.version(), "rates": {}}
    for S in sizes:
        vars_, x0, design, scales = inputs(P, ctx, S)
        lik = P.RNASeqApproxLikelihood(vars_, ctx=ctx)
        regs = {"a": P.RNASeqTranscriptLinearRegression(lik, x0, design, scales, True, 1e-3, False, ctx=ctx)}
        if not only_a:
            rng = np.random.default_rng(1)
            z0 = rng.normal(0, 0.1, size=(S, C_DIM)).astype(np.float32)
            regs["c"] = P.RNASeqTranscriptLinearRegression(lik, x0, design, scales, True, 1e-3, False, ctx=ctx)
            regs["c"].set_latent_design(z0, 1.0)
        for reg in regs.values():  # warm-up: the direct first step, the capture, a few replays
            reg._fit_steps(20, 11)
        rates = {k: [] for k in regs}
        for _ in range(reps):
            for k, reg in regs.items():
                rates[k].append(timed(ctx, reg, STEPS[S]))
        out["rates"][str(S)] = rates
        del regs
    if not only_a and 6 in sizes:
        vars_, x0, _, scales = inputs(P, ctx, 6)
        pca = P.RNASeqPCA(vars_, x0, scales, False, latent_dimensionality=C_DIM, ctx=ctx)
        ctx.synchronize()
        t0 = time.perf_counter()
        _, _, trace = pca.fit(12000, return_trace=True)
        out["pca_fit_12000_s"] = time.perf_counter() - t0
        out["pca_fit_finite"] = bool(np.all(np.isfinite(trace)))
    return out


def child(lib, sizes, reps, only_a):
    """one measuring process (this one only orchestrates and never opens the GPU)"""
    env = dict(os.environ)
    if lib:
        env["POLEE_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--json", "--reps", str(reps), "--sizes", ",".join(map(str, sizes))]
    if only_a:
        cmd.append("--only-a")
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, check=True, timeout=900)
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="6,64")
    ap.add_argument("--out")
    ap.add_argument("--parent-lib")
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.json:
        print(json.dumps(run(sizes, a.reps, a.only_a)))
        return 0
    before = child(a.parent_lib, sizes, a.reps, True) if a.parent_lib else None
    here = child(None, sizes, a.reps, a.only_a)
    after = child(a.parent_lib, sizes, a.reps, True) if a.parent_lib else None
    lines = ["pca_step_rate: n = %d, C = %d, steps/s, median [min .. max] of %d interleaved repetitions" % (N, C_DIM, a.reps),
             "build: " + here["build"]]
    if before:
        lines.append("parent build: " + before["build"])

    def row(label, r):
        return "  %-58s %9.1f  [%9.1f .. %9.1f]" % (label, np.median(r), min(r), max(r))
    for S in sizes:
        r = here["rates"][str(S)]
        lines.append("S = %d (%d steps per timing)" % (S, STEPS[S]))
        if before:
            lines.append(row("(a) plain step, parent build, before", before["rates"][str(S)]["a"]))
            lines.append(row("(a) plain step, parent build, after", after["rates"][str(S)]["a"]))
        lines.append(row("(a) plain step, this build", r["a"]))
        if "c" in r:
            lines.append(row("(c) latent step", r["c"]))
            ma, mc = (np.median(r[k]) for k in "ac")
            lines.append("  us per step over (a): %+.1f" % (1e6 / mc - 1e6 / ma))
    if "pca_fit_12000_s" in here:
        lines.append("RNASeqPCA.fit(12000) at S = 6: %.2f s wall (trace finite: %s)" % (here["pca_fit_12000_s"], here["pca_fit_finite"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

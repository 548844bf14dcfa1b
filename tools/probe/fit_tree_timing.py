"""Phase times of `polee fit-tree` at transcriptome size: a generated transcriptome (tools/synth_seq.py; default n = 200 000,
mean 2 kb), the device path (polee_fit_tree: upload, sketch kernel, candidate edges, host merge -- the builder's own phases,
POLEE_BUILD_TIMING, on stderr) and the --host path (polee_kmer_sketch_host + polee_kmer_tree_host on the host threads), each
--repeat times, and whether both give the same tree.  --merge rounds: the rounds merge on the device (polee_fit_tree_rounds) and its
twin on the host threads (polee_kmer_tree_rounds_host), with the rounds, merges and re-evaluated pairs of each.

    POLEE_BUILD_TIMING=1 python tools/probe/fit_tree_timing.py [--n 200000] [--mean-len 2000] [--seed 1] [--skip-host]
                                                                [--merge {greedy,rounds}] [--repeat 1]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--mean-len", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-device", action="store_true")
    ap.add_argument("--merge", choices=("greedy", "rounds"), default="greedy")
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    import polee_amd as P
    from tools import synth_seq
    t0 = time.time()
    seqs = synth_seq.make_transcripts(a.n, seed=a.seed, mean_len=a.mean_len)
    total = sum(len(s) for s in seqs)
    print("generated n = %d, %d bases (mean %.0f, longest %d) in %.1f s" % (a.n, total, total / a.n, max(map(len, seqs)), time.time() - t0), flush=True)
    trees = {}
    if not a.skip_device:
        ctx = P.Context(0)
        P.kmer_sketches(seqs[:1000], ctx=ctx)  # (first use: module load, the context's first allocations)
        for _ in range(a.repeat):
            stats = {}
            t0 = time.time()
            trees["device"] = P.build_polya_tree_transformation(seqs, ctx=ctx, merge=a.merge, stats=stats)
            print("device path (polee_fit_tree%s, with the concatenation of the sequences): %.3f s %s"
                  % ("_rounds" if a.merge == "rounds" else "", time.time() - t0, stats or ""), flush=True)
    if not a.skip_host:
        t0 = time.time()
        sk = P.kmer_sketches(seqs, host=True)
        t1 = time.time()
        print("host path: sketches %.3f s" % (t1 - t0), flush=True)
        for _ in range(a.repeat):
            stats = {}
            t1 = time.time()
            trees["host"] = P.kmer_tree(sk, host=True, merge=a.merge, stats=stats)
            print("host path: tree (%s) %.3f s (POLEE_HOST_THREADS=%s, %d CPUs usable) %s"
                  % (a.merge, time.time() - t1, os.environ.get("POLEE_HOST_THREADS", "unset"), len(os.sched_getaffinity(0)), stats or ""), flush=True)
        filled = (sk != 0).sum(axis=1)
        print("sketches: %.1f non-empty bins on average, %d empty sketches" % (filled.mean(), int((filled == 0).sum())))
    if len(trees) == 2:
        same = all(np.array_equal(x, y) for x, y in zip(trees["device"], trees["host"]))
        print("device tree == host tree: %s" % same)
        return 0 if same else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

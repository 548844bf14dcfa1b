"""One training of the fragment model from alignment pairs (polee_amd.fragmodel.train_fragment_model) at the reference's size: 200 000
synthetic alignment pairs on 3000 transcripts (tools/synth_aln.py), sequences from make_bias_model.  Prints the wall clock of every
phase (also on stderr with POLEE_BUILD_TIMING=1) and the kernel times of the X build.  One run per figure: no spread is known.

    POLEE_BUILD_TIMING=1 python tools/probe/fragmodel_timing.py [--n 3000] [--m 200000] [--seed 1] [--mixture optimize|em]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import polee_amd as P  # noqa: E402
from polee_amd import fragmodel as FM  # noqa: E402
from tools import synth_aln  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mixture", default="optimize")
    a = ap.parse_args()
    d = synth_aln.make(a.n, a.m, seed=a.seed)
    T, F = d["transcripts"], d["fragments"]
    toy = synth_aln.make_bias_model(T, F, synth_aln.fraglen_model()[0], seed=a.seed + 10)
    ctx = P.Context(0)
    # warm-up: the first call of every kernel loads its code object
    small = synth_aln.make(60, 2000, seed=a.seed)
    toy_small = synth_aln.make_bias_model(small["transcripts"], small["fragments"], synth_aln.fraglen_model()[0], seed=a.seed + 10)
    FM.train_fragment_model(small["transcripts"], small["fragments"], toy_small["tseq_ptr"], toy_small["tseq"], toy_small["m1_reverse"],
                            mixture=a.mixture, ctx=ctx)
    sys.stderr.write("---- warm-up done ----\n")
    t0 = time.perf_counter()
    out = FM.train_fragment_model(T, F, toy["tseq_ptr"], toy["tseq"], toy["m1_reverse"], mixture=a.mixture, seed=a.seed, ctx=ctx)
    wall = time.perf_counter() - t0
    diag = out["diagnostics"]
    print("n %d, m %d, training fragments %d, rows %d, non-zeros %d, mixture %s" % (a.n, a.m, len(diag["indices"]), diag["rows"], diag["nnz"], a.mixture))
    print("counts", diag["counts"])
    for name, s in diag["seconds"].items():
        print("  %-18s %9.3f s" % (name, s))
    print("  %-18s %9.3f s" % ("all", wall))
    truth = d["true_transcript"][diag["indices"]][diag["row_fragment"]]
    print("share of rows assigned to the true transcript %.4f; bias model accuracy %.4f; strand specificity %.4f (simplistic %.4f); median %d (simplistic %d)" % (
        float((diag["transcript"] == truth).mean()), out["bias"]["accuracy"], out["bias"]["strand_specificity"],
        out["fragmodel"]["strand_specificity"], out["bias"]["fraglen_median"], out["fragmodel"]["fraglen_median"]))
    # the two kernels alone, wall clock around the calls (validation, uploads, kernel, downloads)
    sub, idx = FM.subsample_fragments(F, seed=a.seed)
    t0 = time.perf_counter()
    FM.fragmodel_counts(T, sub, ctx)
    print("polee_fragmodel_estimate, call: %.4f s" % (time.perf_counter() - t0))


if __name__ == "__main__":
    main()

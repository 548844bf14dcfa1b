"""One measurement of the splicing features (polee_amd/splicing.py) at annotation size: a generated annotation (tools/synth_annotation.py),
the device path and the host twin on POLEE_HOST_THREADS (default here: 16), phase times from POLEE_BUILD_TIMING=1 on stderr.

    python tools/probe/splicing_timing.py -n 200000 --seed 1 2>&1 | tee profiles/splicing_features_timing.txt"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
os.environ.setdefault("POLEE_HOST_THREADS", "16")

import numpy as np  # noqa: E402

import synth_annotation  # noqa: E402
from polee_amd import splicing  # noqa: E402
from polee_amd.core import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-n", "--num-transcripts", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    t0 = time.perf_counter()
    T = synth_annotation.generate(a.num_transcripts, a.seed)
    print("generated n = %d transcripts, %d exons, %d genes in %.1f s" % (T["n"], len(T["exon_first"]), int(T["gene_of"].max()),
                                                                         time.perf_counter() - t0), flush=True)
    ctx = Context(0)
    warm = synth_annotation.generate(2000, a.seed)
    splicing.splicing_features(warm, warm["gene_of"], ctx=ctx)  # (loads the kernels)
    os.environ["POLEE_BUILD_TIMING"] = "1"
    res = {}
    for name, host in (("device path", False), ("host twin, %s threads" % os.environ["POLEE_HOST_THREADS"], True)):
        print("== %s" % name, flush=True)
        t0 = time.perf_counter()
        r = res[host] = splicing.splicing_features(T, T["gene_of"], host=host, ctx=ctx)
        dt = time.perf_counter() - t0
        sys.stderr.flush()
        print("%s: %.3f s a call; %d features (per type %s), %d internal exons, %d overlapping pairs, %d included + %d excluded members"
              % (name, dt, r["num_features"], np.bincount(r["type"], minlength=7).tolist(), r["num_internal_exons"], r["num_overlapping_pairs"],
                 len(r["included_idx"]), len(r["excluded_idx"])), flush=True)
    keys = ("type", "seq", "strand", "coords", "end_span", "included_ptr", "included_idx", "excluded_ptr", "excluded_idx")
    print("device and host arrays equal:", all(np.array_equal(res[False][k], res[True][k]) for k in keys))


if __name__ == "__main__":
    main()

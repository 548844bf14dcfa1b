"""One timed build of the forest of `polee model random-forest`.

    python tools/probe/forest_timing.py [--device] [--host] [--trees 200] [--out profiles/forest_timing.txt]

N = 1000 rows, n = 200 000 features, k = 3, 200 trees, nsub = 4472 candidate features per node: rows N(0,1), class c adds 2.0 on its
own 50 features.  --device times RNASeqRandomForest.fit on points (host clock around the call, upload included; a small warm-up fit
first) and the votes on the training rows; --host times the host builder on POLEE_HOST_THREADS threads.  With both, the two forests
are compared node for node.  The device's share by kernel comes from a kernel trace of `--device` alone (rocprofv3 --kernel-trace
--stats -- python tools/probe/forest_timing.py --device), not from this script.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, FEATURES, K, SIGNAL = 1000, 200000, 3, 50


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    from polee_amd import random_forest as RF
    rng = np.random.default_rng(0)
    y = rng.integers(0, K, N).astype(np.int32)
    x = rng.standard_normal((N, FEATURES), dtype=np.float32)
    for c in range(K):
        x[np.ix_(y == c, np.arange(c * SIGNAL, (c + 1) * SIGNAL))] += np.float32(2.0)
    lines = ["N = %d, n = %d, k = %d, %d trees, nsub = %d" % (N, FEATURES, K, a.trees, RF.forest_opts().nsubfeatures * FEATURES ** 0.5)]
    dev = host = None
    if a.device:
        import polee_amd as P
        ctx = P.Context(0)
        RF.RNASeqRandomForest(K, 64, ctx=ctx, ntrees=4).fit(x[:100, :64].copy(), y[:100], seed=1)  # warm-up
        f = RF.RNASeqRandomForest(K, FEATURES, ctx=ctx, ntrees=a.trees)
        t0 = time.perf_counter()
        f.fit(x, y, seed=7)
        t1 = time.perf_counter()
        v = f.votes(x)
        t2 = time.perf_counter()
        dev = f.nodes()
        depth = max(RF_depth(dev, t) for t in range(a.trees))
        lines.append("device fit %.3f s (upload of x included), votes of %d rows %.3f s; %d nodes, deepest tree %d levels, training accuracy %.3f"
                     % (t1 - t0, N, t2 - t1, len(dev[1]), depth, float((v.argmax(axis=1) == y).mean())))
    if a.host:
        t0 = time.perf_counter()
        host = RF.build_forest_host(x, y, K, 7, ntrees=a.trees)
        t1 = time.perf_counter()
        lines.append("host build %.3f s on POLEE_HOST_THREADS=%s; %d nodes" % (t1 - t0, os.environ.get("POLEE_HOST_THREADS", "(unset)"), len(host[1])))
    if dev is not None and host is not None:
        same = all(np.array_equal(u, v) for u, v in zip(dev, host))
        lines.append("device forest == host forest: %s" % same)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


def RF_depth(nodes, t):
    off, feature, _, left, right, _ = nodes
    b, depth, level = int(off[t]), 0, [0]
    while True:
        level = [c for i in level if feature[b + i] >= 0 for c in (left[b + i], right[b + i])]
        if not level:
            return depth
        depth += 1


if __name__ == "__main__":
    main()

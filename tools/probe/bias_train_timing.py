"""One timed training of the bias model at the reference's size (profiles/bias_train_timing.txt): 200 000 foreground + 200 000 drawn
background fragments of 150 .. 400 bases on 3000 transcripts, examples + both ends + GC + accuracy; the device path and, with --host,
the host trainer on POLEE_HOST_THREADS.  Foreground positions are accepted more often when the three bases around the fragment's
start and the base at its end are C or G, so that the search has rounds to commit.

    python tools/probe/bias_train_timing.py [--host] [--no-device]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from polee_amd import bias as B  # noqa: E402


def make(n_t=3000, n_fg=200000, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(500, 3000, n_t)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tseq = rng.integers(0, 4, ptr[-1]).astype(np.uint8)
    t = rng.integers(0, n_t, 4 * n_fg).astype(np.int32)
    fl = rng.integers(150, 401, len(t)).astype(np.int32)
    pos = (1 + np.floor(rng.random(len(t)) * (lens[t] - fl + 1))).astype(np.int64)
    gc = lambda off: np.isin(tseq[np.clip(ptr[t] + pos - 1 + off, ptr[t], ptr[t + 1] - 1)], (1, 2))
    w = 0.15 + 0.2 * gc(0) + 0.2 * (gc(0) & gc(1)) + 0.15 * gc(-1) + 0.3 * gc(fl - 1)
    keep = np.flatnonzero(rng.random(len(t)) < w)[:n_fg]
    assert len(keep) == n_fg
    return ptr, tseq, t[keep], pos[keep], fl[keep]


def run(data, host, ctx):
    t0 = time.perf_counter()
    bt, dropped = B.bias_trainer(*data, seed=7, host=host, ctx=ctx)
    t1 = time.perf_counter()
    with bt:
        m = bt.run().model()
    t2 = time.perf_counter()
    return m, t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    a = ap.parse_args()
    data = make()
    print("%d transcripts, %d bases, %d + %d fragments" % (len(data[0]) - 1, data[0][-1], len(data[2]), len(data[2])), flush=True)
    models = {}
    if not a.no_device:
        import polee_amd as P
        ctx = P.Context(0)
        small = tuple(x[:2000] if i >= 2 else x for i, x in enumerate(data))
        run(small, False, ctx)  # warm-up: code objects loaded, buffers cached
        m, tc, tr = run(data, False, ctx)
        models["device"] = m
        print("device: examples %.3f s, training %.3f s; rounds left %d right %d; accuracy %.4f" % (
            tc, tr, len(m["loss_trace_left"]) - 1, len(m["loss_trace_right"]) - 1, m["accuracy"]), flush=True)
        print("  orders left %s\n  orders right %s" % (m["orders_left"].tolist(), m["orders_right"].tolist()), flush=True)
    if a.host:
        m, tc, tr = run(data, True, None)
        models["host"] = m
        print("host (POLEE_HOST_THREADS=%s): examples %.3f s, training %.3f s; rounds left %d right %d; accuracy %.4f" % (
            os.environ.get("POLEE_HOST_THREADS", "unset"), tc, tr, len(m["loss_trace_left"]) - 1, len(m["loss_trace_right"]) - 1,
            m["accuracy"]), flush=True)
    if len(models) == 2:
        d, h = models["device"], models["host"]
        same = all(np.array_equal(np.asarray(d[k]).view(np.uint32), np.asarray(h[k]).view(np.uint32))
                   for k in ("orders_left", "orders_right", "ps_left", "ps_right", "gc_bins")) and d["accuracy"] == h["accuracy"]
        dev = max(float(np.max(np.abs(d[k] - h[k]) / np.abs(h[k]))) for k in ("loss_trace_left", "loss_trace_right")
                  if len(d[k]) == len(h[k]))
        print("device model == host model: %s; largest relative deviation of the loss traces %.3g" % (same, dev), flush=True)


if __name__ == "__main__":
    main()

"""Gibbs sampler (csrc/gibbs.hip) throughput: sweeps/s for C = 1, 8, 32 chains at C2 (literal and patterns generators) and on the
real fixture tiled x639; the bytes a sweep must read and the fraction of HBM peak; polee_gibbs_create time (from Xt); the
end-to-end time of `python -m polee_amd.gibbs` with the reference defaults at C2 (literal); the NumPy restatement's sweeps/s at
fixture size (16 chains) as the CPU point.  Output: one line per measurement on stdout.
GIBBS_BENCH_SWEEPS (default 100) timed sweeps per point; GIBBS_BENCH_QUICK=1: C = 8 at C2 literal only (the profiler run)."""
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import polee_amd as P  # noqa: E402
from polee_amd.gibbs import GibbsSampler  # noqa: E402
from tools import synth  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X
N, M = 200_000, 30_000_000
K = int(os.environ.get("GIBBS_BENCH_SWEEPS", "100"))
QUICK = os.environ.get("GIBBS_BENCH_QUICK") == "1"


def sweep_bytes(info, C):
    """What one sweep must move at least: the rows once (col + val, row offsets, original index, tile windows), the chains' state
    (g read by the gathers and written by the draw, this sweep's counts read, the other buffer cleared), the base counts."""
    M_, nnz, n, T = info["num_multi_rows"], info["multi_nnz"], info["n"], info["num_tiles"]
    x = 8 * nnz + 4 * (M_ + 1) + 4 * M_ + 8 * T
    state = 4 * n * C * 4 + 4 * n
    return x + state


def bench(name, smp, Cs):
    ctx = P.Context(0)
    for C in Cs:
        t0 = time.time()
        g = GibbsSampler(smp["m"], smp["n"], None, None, None, smp["effective_lengths"], C, 1, ctx=ctx,
                         xt=(smp["tcolptr"], smp["trowval"], smp["tnzval"]))
        t_create = time.time() - t0
        info = g.info
        g.run(5, 0)
        g.sync()
        ctx.timer_start()
        g.run(K, 0)
        ms = ctx.timer_stop() / K
        g.sync()
        b = sweep_bytes(info, C)
        print("%-12s C=%-2d  %.3f ms/sweep  %8.1f sweeps/s  bytes/sweep %.3f GB  %.1f %% of HBM peak  create %.3f s  "
              "(multi rows %d, single %d, empty %d, multi nnz %d, tiles %d)"
              % (name, C, ms, 1e3 / ms, b / 1e9, 100 * b / (ms * 1e-3) / HBM_PEAK, t_create, info["num_multi_rows"],
                 info["num_single_rows"], info["num_empty_rows"], info["multi_nnz"], info["num_tiles"]), flush=True)
        del g


def end_to_end(smp):
    """The CLI with the reference defaults (2 000 burn-in, 1 000 samples, stride 25, 8 chains, kallisto output) on a C2 file."""
    tmp = tempfile.mkdtemp(prefix="gibbs_e2e_")
    try:
        need = 12 * smp["nnz"] + 2 * 8 * N * 1000 + (1 << 30)
        if shutil.disk_usage(tmp).free < need:
            print("end-to-end: skipped (%.1f GB free, %.1f GB needed)" % (shutil.disk_usage(tmp).free / 1e9, need / 1e9), flush=True)
            return
        from polee_amd import h5io
        colptr, rowval, nzval = synth.to_csc(smp)
        lm = os.path.join(tmp, "c2.likelihood-matrix.h5")
        with h5io.File(lm, "w") as f:  # (uncompressed: the writer's deflate would dominate the setup)
            f.write("m", np.int64(smp["m"]))
            f.write("n", np.int64(smp["n"]))
            f.write("colptr", colptr.astype(np.uint32))
            f.write("rowval", rowval)
            f.write("nzval", nzval)
            f.write("effective_lengths", smp["effective_lengths"])
            f.create_group("metadata")
        out = os.path.join(tmp, "g.h5")
        t0 = time.time()
        subprocess.check_call([sys.executable, "-m", "polee_amd.gibbs", lm, "-o", out, "--kallisto"], cwd=ROOT,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        dt = time.time() - t0
        print("end-to-end python -m polee_amd.gibbs --kallisto at C2 literal, reference defaults (5 125 sweeps, 8 chains, "
              "1 000 draws written): %.1f s (output %.2f GB)" % (dt, os.path.getsize(out) / 1e9), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def cpu_point():
    from test_gibbs_host import Layout, NumpyGibbs, rows_of
    a = np.load(os.path.join(ROOT, "tests", "golden", "mBr_M_6w_1.likelihood-matrix.npz"))
    m, n = int(a["m"][0]), int(a["n"][0])
    lay = Layout(m, n, *rows_of(m, n, a["colptr"], a["rowval"], a["nzval"]))
    s = NumpyGibbs(lay, 16, seed=1)
    s.step()
    t0 = time.time()
    for _ in range(30):
        s.step()
    dt = (time.time() - t0) / 30
    print("cpu NumPy restatement, fixture (m = %d, n = %d), 16 chains: %.1f sweeps/s" % (m, n, 1 / dt), flush=True)


def main():
    lit = synth.make_sample(N, M, 8.0, seed=123456789, literal=True)
    bench("c2-literal", lit, (8,) if QUICK else (1, 8, 32))
    if QUICK:
        return
    bench("c2-patterns", synth.make_sample(N, M, 8.0, seed=123456789), (1, 8, 32))
    bench("fixture-x639", synth.tile_fixture(639), (1, 8, 32))
    end_to_end(lit)
    cpu_point()


if __name__ == "__main__":
    main()

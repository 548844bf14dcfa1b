"""EM maximum-likelihood estimate of the transcript mixture of a likelihood matrix: `polee debug-optimize` (src/main.jl:960-988
handler; expectation_maximization, src/em.jl:3-87).  The iterations run in libpolee_hip.so (csrc/em.hip) on the likelihood
handle of a core.RNASeqSample; this module does the I/O, the arguments and the CSV.

    python -m polee_amd.em likelihood-matrix.h5 [-o em.csv] [--max-iters N] [--tol EPS] [--check-every N] [--no-efflen]
        [--deterministic] [--transcript-ids ids.txt] [--trace trace.csv]

The reference names transcripts from --annotations / --sequences; GFF and FASTA parsing is out of scope here, so the ids come
from a text file with one id per line (--transcript-ids, default 1..n), as in polee_amd.gibbs.  --trace writes the
log-likelihood of every iterate (the reference prints it, em.jl:74).

The stop rule is the reference's (em.jl:76): stop with the first iterate whose log-likelihood gains less than --tol (1e-6).  The
log-likelihood is summed in f64 here, but the iterates are f32, and their rounding moves lp by about 3e-11 of |lp| from one
iterate to the next: 1e-5 on the reference's fixture, 1e-2 at 30 M fragments.  Below that floor the rule fires on noise, not on
convergence: with the defaults the fixture stops after 786 iterations where the exact increase is still 8e-6, and a 30 M-fragment
sample stops on a DEcrease, after 285 iterations in one run and 316 in the next.  The iteration count of a default run is
therefore not reproducible from run to run unless --deterministic fixes the summation order; a run that is to go further takes
--tol -1 and --max-iters.  Other deviations from em.jl: fragments compatible with no transcript are dropped
instead of giving log 0; the output defaults to em.csv."""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib as L
from . import h5io
from ._lib import check, ptr, f32p, f64p

DEFAULT_TOL = 1e-6  # em.jl:39
DEFAULT_MAX_ITERS = 5000
DEFAULT_CHECK_EVERY = 64


class EMInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("M", C.c_int64), ("iters", C.c_int64), ("converged", C.c_int32), ("nonfinite", C.c_int32),
                ("lp_start", C.c_double), ("last_lp", C.c_double), ("last_increase", C.c_double), ("sum_y", C.c_double),
                ("kkt_max", C.c_double)]


def _start(y0, n):
    if y0 is None:
        return None
    y = np.ascontiguousarray(y0, np.float32)
    if y.shape != (n,):
        raise ValueError("y0: %s given for %d transcripts" % (y.shape, n))
    return y


class EM(L.Handle):
    """EM over the X of an existing core.RNASeqSample (polee_em): its device layout, its multiplicities ks and its effective
    lengths are used as they are.  While iterations run, nothing else may evaluate the same sample (one evaluation slot per
    likelihood handle)."""
    _destroy = "polee_em_destroy"

    def __init__(self, sample, y0=None):
        self.sample, self.ctx, self.n = sample, sample.ctx, int(sample.n)
        self._h = C.c_void_p()
        y = _start(y0, self.n)
        check(L.lib().polee_em_create(sample._h, ptr(y, f32p), C.byref(self._h)), self.ctx._h)

    def reset(self, y0=None):
        y = _start(y0, self.n)
        check(L.lib().polee_em_reset(self._h, ptr(y, f32p)), self.ctx._h)

    def run(self, max_iters=DEFAULT_MAX_ITERS, tol=DEFAULT_TOL, check_every=DEFAULT_CHECK_EVERY):
        """Up to max_iters more iterations; stops with the first iterate whose log-likelihood gains less than tol (tol < 0:
        never).  Returns info."""
        check(L.lib().polee_em_run(self._h, C.c_int32(int(max_iters)), C.c_double(float(tol)), C.c_int32(int(check_every))),
              self.ctx._h)
        return self.info()

    def sync(self):
        check(L.lib().polee_em_sync(self._h), self.ctx._h)

    def mixture(self):
        y = np.empty(self.n, np.float32)
        check(L.lib().polee_em_get_mixture(self._h, ptr(y, f32p)), self.ctx._h)
        return y

    def tpm(self, use_efflen=True, efflens=None):
        """1e6 (y / l) / sum(y / l) with the sample's effective lengths (or `efflens`); use_efflen=False: 1e6 y."""
        el = None
        if use_efflen:
            el = self.sample.effective_lengths if efflens is None else efflens
            if el is None:
                raise ValueError("the sample has no effective lengths (pass efflens or use_efflen=False)")
            el = np.ascontiguousarray(el, np.float32)
            if el.shape != (self.n,):
                raise ValueError("efflens: %s given for %d transcripts" % (el.shape, self.n))
        out = np.empty(self.n, np.float32)
        check(L.lib().polee_em_get_tpm(self._h, ptr(el, f32p), ptr(out, f32p)), self.ctx._h)
        return out

    def trace(self):
        """Log-likelihood of iterates 1, 2, ... -> f64 [iterations]."""
        k = C.c_int64()
        check(L.lib().polee_em_get_trace(self._h, None, C.c_int64(0), C.byref(k)), self.ctx._h)
        lp = np.empty(k.value, np.float64)
        check(L.lib().polee_em_get_trace(self._h, ptr(lp, f64p), C.c_int64(lp.size), C.byref(k)), self.ctx._h)
        return lp[:k.value]

    def info(self, kkt=False):
        i = EMInfo()
        check(L.lib().polee_em_get_info(self._h, C.c_int(int(bool(kkt))), C.byref(i)), self.ctx._h)
        return {k: getattr(i, k) for k, _ in i._fields_}


def write_csv(output_filename, transcript_ids, tpms):
    """main.jl:982-987: `transcript_id,tpm`, then one line per transcript (Float32 printed as Julia's println does)."""
    tpms = np.asarray(tpms, np.float32)
    if len(transcript_ids) != tpms.size:
        raise ValueError("Likelihood matrix has different number of transcripts than annotations.")
    with open(output_filename, "w") as out:
        out.write("transcript_id,tpm\n")
        for name, v in zip(transcript_ids, tpms):
            out.write("%s,%s\n" % (name, _julia_f32(v)))


def _julia_f32(v):
    """The shortest decimal that reads back as the same Float32, in Julia's print form (1.0e-5, 12.5, 3.0f8 is not used by print)."""
    v = np.float32(v)
    if not np.isfinite(v):
        return "NaN" if np.isnan(v) else ("Inf" if v > 0 else "-Inf")
    if v == 0:
        return "0.0"
    a = abs(float(v))
    if 1e-5 <= a < 1e6:
        s = np.format_float_positional(v, unique=True, trim="0")
        return s if "." in s else s + ".0"
    s = np.format_float_scientific(v, unique=True, trim="0", exp_digits=1)
    mant, exp = s.split("e")
    if "." not in mant:
        mant += ".0"
    return "%se%d" % (mant, int(exp))


def write_trace_csv(output_filename, lp):
    with open(output_filename, "w") as out:
        out.write("iteration,lp\n")
        for t, v in enumerate(np.asarray(lp, np.float64), start=1):
            out.write("%d,%.17g\n" % (t, v))


def _check_run_args(max_iters, check_every):
    if max_iters < 1:
        raise ValueError("max_iters must be at least 1 (got %d)" % max_iters)
    if check_every < 1:
        raise ValueError("check_every must be at least 1 (got %d)" % check_every)


def _run(lm, max_iters, tol, check_every, deterministic, ctx=None):
    """The sample of a likelihood matrix as read from its HDF5, and its EM after one run."""
    _check_run_args(max_iters, check_every)
    from .core import RNASeqSample
    sample = RNASeqSample(lm["m"], lm["n"], lm["colptr"], lm["rowval"], lm["nzval"], lm["effective_lengths"], ctx=ctx)
    if deterministic:
        sample.set_deterministic(True)
    em = EM(sample)
    em.run(max_iters, tol, check_every)
    return em


def expectation_maximization(likelihood_matrix_filename, max_iters=DEFAULT_MAX_ITERS, tol=DEFAULT_TOL,
                             check_every=DEFAULT_CHECK_EVERY, use_efflen=True, deterministic=False, ctx=None):
    """expectation_maximization (em.jl:3-87) on the GPU: the TPM vector, f32 [n].  With the default tol the run ends where the
    iterates' f32 rounding hides the increase (see the module's text); tol < 0 runs exactly max_iters iterations."""
    _check_run_args(max_iters, check_every)
    lm = h5io.read_likelihood_matrix(likelihood_matrix_filename)
    return _run(lm, max_iters, tol, check_every, deterministic, ctx).tpm(use_efflen)


def _read_lines(filename):
    with open(filename) as f:
        return [line.strip() for line in f if line.strip()]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    ap = argparse.ArgumentParser(prog="python -m polee_amd.em", description=__doc__.split("\n\n")[0])
    ap.add_argument("likelihood_matrix", metavar="likelihood-matrix.h5")
    ap.add_argument("--output", "-o", default="em.csv", help="Output CSV (transcript_id,tpm); default em.csv.")
    ap.add_argument("--max-iters", type=int, default=DEFAULT_MAX_ITERS, metavar="N", help="Most iterations to run.")
    ap.add_argument("--tol", type=float, default=DEFAULT_TOL, metavar="EPS",
                    help="Stop when the log-likelihood gains less than this (negative: run --max-iters iterations).  Below about 3e-11 of "
                         "|lp| -- the f32 rounding of the iterates -- the rule fires on noise, and where it does varies from run to run "
                         "without --deterministic.")
    ap.add_argument("--check-every", type=int, default=DEFAULT_CHECK_EVERY, metavar="N",
                    help="Iterations queued between two reads of the stop flag.")
    ap.add_argument("--no-efflen", action="store_true", help="Do not do effective length transformation.")
    ap.add_argument("--deterministic", action="store_true", help="Fixed summation order: a bitwise reproducible estimate and iteration count.")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (default 1..n).")
    ap.add_argument("--trace", metavar="trace.csv", help="Write iteration,lp for every iteration.")
    a = ap.parse_args(argv)
    try:
        _check_run_args(a.max_iters, a.check_every)
    except ValueError as e:
        ap.error(str(e))
    lm = h5io.read_likelihood_matrix(a.likelihood_matrix)
    n = lm["n"]
    ids = _read_lines(a.transcript_ids) if a.transcript_ids else [str(j) for j in range(1, n + 1)]
    if len(ids) != n:
        ap.error("--transcript-ids: %d ids for %d transcripts" % (len(ids), n))
    em = _run(lm, a.max_iters, a.tol, a.check_every, a.deterministic)
    tpm = em.tpm(not a.no_efflen)
    info = em.info()
    print("EM: %d iterations, %s, lp %.6f (last increase %.3g)" % (info["iters"], "converged" if info["converged"] else
                                                                   "not converged", info["last_lp"], info["last_increase"]),
          file=sys.stderr)
    write_csv(a.output, ids, tpm)
    if a.trace:
        write_trace_csv(a.trace, em.trace())
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Gibbs sampler of the exact posterior of a likelihood matrix: `polee debug-sample` (src/main.jl:291-335 flags, :925-957
handler; src/gibbs.jl).  Collapsed Gibbs sampling over fragment assignments draws the transcript mixture from p(y | X) under a
Dirichlet(1) prior -- the posterior the fitted approximation is judged against.  The sampling runs in libpolee_hip.so
(csrc/gibbs.hip); this module does the I/O, the arguments and the writers' bookkeeping.

    python -m polee_amd.gibbs likelihood-matrix.h5 -o out [--kallisto] [--num-samples N] [--burnin N] [--stride N]
        [--no-efflen] [--seed N] [--chains C] [--transcript-ids ids.txt] [--transcript-lengths lens.txt]

The reference names transcripts from --annotations / --sequences; GFF and FASTA parsing is out of scope here, so the ids come
from a text file with one id per line (--transcript-ids) and the lengths written to the kallisto file from one with one integer
per line (--transcript-lengths).  Without them the ids are 1..n and the lengths -1.  An ids file whose length is not n is an
error, as in gibbs.jl:15-17.

Two reference quirks are fixed on purpose: under --no-efflen the kallisto counts are prop * m (gibbs.jl:113-119
leaves them undefined), and exactly stride * samples_per_chain sweeps are sampled -- the last convergence checkpoint may be
partial (gibbs.jl:86-89 drops the remainder and leaves stored samples uninitialised)."""
import argparse
import ctypes as C
import datetime
import sys

import numpy as np

from . import _lib as L
from . import h5io
from ._lib import arr, check, ptr, f32p, u32p, u64p

DEFAULT_SEED = 123456789  # main.jl:322-326


class GibbsInfo(C.Structure):
    _fields_ = [("m", C.c_int64), ("n", C.c_int64), ("nnz", C.c_int64), ("num_chains", C.c_int32),
                ("num_multi_rows", C.c_int64), ("num_single_rows", C.c_int64), ("num_empty_rows", C.c_int64),
                ("multi_nnz", C.c_int64), ("num_tiles", C.c_int64), ("rows_per_tile", C.c_int32), ("sweeps_done", C.c_int64)]


class GibbsSampler(L.Handle):
    """num_chains collapsed Gibbs chains over X on the GPU (polee_gibbs).  X by columns as in the likelihood-matrix HDF5
    (colptr / rowval 1-based), or fragment-major through xt = (tcolptr u64 [m+1], trowval u32, tnzval f32), 1-based.
    efflens = None: no effective-length transformation of the stored draws (--no-efflen)."""
    _destroy = "polee_gibbs_destroy"

    def __init__(self, m, n, colptr, rowval, nzval, efflens=None, num_chains=8, seed=DEFAULT_SEED, ctx=None, xt=None):
        from .core import default_context
        self.ctx = ctx or default_context()
        self.m, self.n, self.num_chains = int(m), int(n), int(num_chains)
        self._h = C.c_void_p()
        el = None if efflens is None else arr(efflens, np.float32)
        lib = L.lib()
        if xt is not None:
            tp, tr, tv = arr(xt[0], np.uint64), arr(xt[1], np.uint32), arr(xt[2], np.float32)
            check(lib.polee_gibbs_create_from_xt(self.ctx._h, C.c_int64(self.m), C.c_int64(self.n), ptr(tp, u64p), ptr(tr, u32p),
                                                 ptr(tv, f32p), ptr(el, f32p), C.c_int32(self.num_chains), C.c_uint64(int(seed)),
                                                 C.byref(self._h)), self.ctx._h)
        else:
            colptr = np.ascontiguousarray(colptr)
            if colptr.dtype not in (np.dtype(np.uint32), np.dtype(np.uint64)):
                colptr = colptr.astype(np.uint64)
            rowval, nzval = arr(rowval, np.uint32), arr(nzval, np.float32)
            check(lib.polee_gibbs_create(self.ctx._h, C.c_int64(self.m), C.c_int64(self.n), colptr.ctypes.data_as(C.c_void_p),
                                         int(colptr.dtype.itemsize), ptr(rowval, u32p), ptr(nzval, f32p), ptr(el, f32p),
                                         C.c_int32(self.num_chains), C.c_uint64(int(seed)), C.byref(self._h)), self.ctx._h)

    def set_state(self, g0=None):
        """Chains' unnormalised mixture [C, n] (finite, >= 0), or None = fresh Gamma(1) draws."""
        g = None if g0 is None else arr(g0, np.float32).reshape(self.num_chains, self.n)
        check(L.lib().polee_gibbs_set_state(self._h, ptr(g, f32p)), self.ctx._h)

    def reserve(self, draws_per_chain):
        check(L.lib().polee_gibbs_reserve(self._h, C.c_int32(int(draws_per_chain))), self.ctx._h)

    def run(self, nsweeps, stride=0):
        """Queues nsweeps sweeps; stride > 0 stores the state after every stride-th one, 0 = burn-in."""
        check(L.lib().polee_gibbs_run(self._h, C.c_int32(int(nsweeps)), C.c_int32(int(stride))), self.ctx._h)

    def sync(self):
        check(L.lib().polee_gibbs_sync(self._h), self.ctx._h)

    @property
    def num_stored(self):
        k = C.c_int32()
        check(L.lib().polee_gibbs_num_stored(self._h, C.byref(k)), self.ctx._h)
        return k.value

    def get_draws(self, first=0, count=None):
        """Stored draws [first, first + count) -> f32 [C, count, n]."""
        if count is None:
            count = self.num_stored - first
        out = np.empty((self.num_chains, int(count), self.n), np.float32)
        check(L.lib().polee_gibbs_get_draws(self._h, C.c_int32(int(first)), C.c_int32(int(count)), ptr(out, f32p)), self.ctx._h)
        return out

    def get_counts(self):
        """Fragments per transcript in the last sweep, single-transcript fragments included -> u32 [C, n]."""
        out = np.empty((self.num_chains, self.n), np.uint32)
        check(L.lib().polee_gibbs_get_counts(self._h, ptr(out, u32p)), self.ctx._h)
        return out

    def rhat(self):
        """Split-R-hat per transcript over all stored draws (convergence_stats, gibbs.jl:283-319) -> f32 [n]."""
        out = np.empty(self.n, np.float32)
        check(L.lib().polee_gibbs_rhat(self._h, ptr(out, f32p)), self.ctx._h)
        return out

    @property
    def info(self):
        i = GibbsInfo()
        check(L.lib().polee_gibbs_get_info(self._h, C.byref(i)), self.ctx._h)
        return {k: getattr(i, k) for k, _ in i._fields_}

    def debug_assignments(self, chain):
        """Test hook: the 1-based transcript the last sweep gave each fragment of chain `chain` (0 = empty fragment) -> i32 [m]."""
        z = np.empty(self.m, np.int32)
        check(L.lib().polee_debug_gibbs_assignments(self._h, C.c_int32(int(chain)), z.ctypes.data_as(C.POINTER(C.c_int32))),
              self.ctx._h)
        return z


def _prop_to_counts(prop, efflens, m, use_efflen):
    """prop_to_counts (gibbs.jl:113-119): stored draws (efflen-adjusted) back to fragment shares, times m."""
    prop = np.asarray(prop, np.float64)
    if use_efflen:
        p = prop * np.asarray(efflens, np.float64)
        p /= p.sum(axis=-1, keepdims=True)
    else:
        p = prop  # (undefined in the reference: prop_ is never assigned under --no-efflen)
    return p * m


def write_kallisto(output_filename, samples, efflens, m, transcript_ids, transcript_lengths, use_efflen=True, call=""):
    """The kallisto HDF5 layout of gibbs.jl:122-156 for sleuth: samples f32 [C, S, n]."""
    samples = np.asarray(samples)
    Cn, S, n = samples.shape
    with h5io.File(output_filename, "w") as f:
        post_mean = samples.astype(np.float64).mean(axis=(0, 1))
        f.write("est_counts", _prop_to_counts(post_mean, efflens, m, use_efflen))
        f.create_group("aux")
        f.write("aux/num_bootstrap", np.array([Cn * S], np.int64))
        f.write("aux/eff_lengths", np.asarray(efflens, np.float64))
        f.write("aux/lengths", np.asarray(transcript_lengths, np.int64))
        f.write_strings("aux/ids", [str(t) for t in transcript_ids])
        f.write_strings("aux/call", [call])
        f.write("aux/index_version", np.array([-1], np.int64))
        f.write_strings("aux/kallisto_version", "polee debug-sample")
        f.write_strings("aux/start_time", datetime.datetime.now().isoformat())
        f.create_group("bootstrap")
        k = 0
        for c in range(Cn):
            for s in range(S):
                f.write("bootstrap/bs%d" % k, _prop_to_counts(samples[c, s], efflens, m, use_efflen))
                k += 1


def write_csv(output_filename, samples, transcript_ids):
    """gibbs.jl:157-175: a header of transcript ids, then one %e row per draw (chain-major)."""
    samples = np.asarray(samples)
    with open(output_filename, "w") as out:
        out.write(",".join(str(t) for t in transcript_ids) + "\n")
        for c in range(samples.shape[0]):
            for s in range(samples.shape[1]):
                out.write(",".join("%e" % v for v in samples[c, s].tolist()) + "\n")


def _rhat_line(r):
    return ",".join("NaN" if not np.isfinite(v) else str(np.float32(v)) for v in r)


def gibbs_sampler(likelihood_matrix_filename, output_filename, transcript_ids=None, kallisto=False, num_samples=1000,
                  num_burnin_samples=2000, sample_stride=25, convergence_test_stride=125, use_efflen=True, num_chains=8,
                  seed=DEFAULT_SEED, transcript_lengths=None, ctx=None, call="", verbose=False):
    """gibbs_sampler (gibbs.jl:1-177) on the GPU: num_burnin_samples burn-in sweeps, then sample_stride * samples_per_chain sweeps
    (samples_per_chain = num_samples // num_chains) storing every sample_stride-th state, split-R-hat per transcript at every
    convergence_test_stride sweeps into <output_filename>.convergence.csv, the draws to output_filename (kallisto HDF5 or CSV).
    Returns the draws, f32 [num_chains, samples_per_chain, n]."""
    lm = h5io.read_likelihood_matrix(likelihood_matrix_filename)
    m, n = lm["m"], lm["n"]
    if transcript_ids is None:
        transcript_ids = [str(j) for j in range(1, n + 1)]
    transcript_ids = list(transcript_ids)
    if len(transcript_ids) != n:
        raise ValueError("Likelihood matrix has different number of transcripts than annotations.")
    if transcript_lengths is None:
        transcript_lengths = np.full(n, -1, np.int64)
    transcript_lengths = np.asarray(transcript_lengths, np.int64)
    if transcript_lengths.shape != (n,):
        raise ValueError("transcript lengths: %d given for %d transcripts" % (transcript_lengths.size, n))
    if sample_stride < 1 or convergence_test_stride < 1 or num_burnin_samples < 0 or num_samples < 0:
        raise ValueError("strides must be positive and sample counts non-negative")
    samples_per_chain = num_samples // num_chains
    els = lm["effective_lengths"]
    g = GibbsSampler(m, n, lm["colptr"], lm["rowval"], lm["nzval"], els if use_efflen else None, num_chains, seed, ctx=ctx)
    g.reserve(samples_per_chain)
    g.run(num_burnin_samples, 0)
    total = sample_stride * samples_per_chain
    with open(output_filename + ".convergence.csv", "w") as diag:
        done = 0
        while done < total:
            k = min(convergence_test_stride, total - done)
            g.run(k, sample_stride)
            done += k
            r = g.rhat() if g.num_stored > 0 else np.full(n, np.nan, np.float32)
            if verbose:
                q = np.quantile(r[np.isfinite(r)], [0.0, 1e-3, 1e-2, 0.5, 0.99, 0.999, 1.0]) if np.isfinite(r).any() else []
                print("Sampling: %d/%d  R-hat quantiles %s" % (done, total, np.array2string(np.asarray(q), precision=4)),
                      file=sys.stderr)
            diag.write(_rhat_line(r) + "\n")
    g.sync()
    samples = g.get_draws()
    if kallisto:
        write_kallisto(output_filename, samples, els, m, transcript_ids, transcript_lengths, use_efflen, call)
    else:
        write_csv(output_filename, samples, transcript_ids)
    return samples


def _read_lines(filename):
    with open(filename) as f:
        return [line.strip() for line in f if line.strip()]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    ap = argparse.ArgumentParser(prog="python -m polee_amd.gibbs", description=__doc__.split("\n\n")[0])
    ap.add_argument("likelihood_matrix", metavar="likelihood-matrix.h5")
    ap.add_argument("--output", "-o")
    ap.add_argument("--kallisto", action="store_true", help="Output samples in a format compatible with kallisto, for use with sleuth.")
    ap.add_argument("--num-samples", type=int, default=1000, metavar="N", help="Number of samples to generate and record.")
    ap.add_argument("--stride", type=int, default=25, metavar="N", help="Number of samples to generate and not record for each recorded sample.")
    ap.add_argument("--burnin", type=int, default=2000, metavar="N", help="Number of initialization samples to generate.")
    ap.add_argument("--no-efflen", action="store_true", help="Do not do effective length transformation.")
    ap.add_argument("--seed", type=int, default=DEFAULT_SEED, metavar="N", help="RNG seed")
    ap.add_argument("--chains", type=int, default=8, metavar="C", help="Number of chains (1..32; the reference runs one per thread).")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (default 1..n).")
    ap.add_argument("--transcript-lengths", metavar="lens.txt", help="Transcript lengths, one per line (default -1).")
    a = ap.parse_args(argv)
    out = a.output if a.output is not None else ("gibbs-samples.h5" if a.kallisto else "gibbs-samples.csv")
    ids = _read_lines(a.transcript_ids) if a.transcript_ids else None
    lens = np.array([int(v) for v in _read_lines(a.transcript_lengths)], np.int64) if a.transcript_lengths else None
    gibbs_sampler(a.likelihood_matrix, out, transcript_ids=ids, kallisto=a.kallisto, num_samples=a.num_samples,
                  num_burnin_samples=a.burnin, sample_stride=a.stride, use_efflen=not a.no_efflen, num_chains=a.chains, seed=a.seed,
                  transcript_lengths=lens, call=" ".join(argv), verbose=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

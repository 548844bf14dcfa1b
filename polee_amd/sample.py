"""Draws from a fitted approximation: `polee sample` (src/main.jl:239-289 flags, :756-919 handler).  A prepared sample becomes
posterior-mean TPMs (CSV) or a kallisto-style bootstrap file for sleuth (HDF5).  The draws, the effective-length adjustment, the
running posterior mean and prop_to_counts -- expected counts, or with --sample-counts an exact multinomial draw of the m reads --
run in libpolee_hip.so (csrc/sample.hip); this module does the I/O, the arguments and the writers' bookkeeping.

    python -m polee_amd.sample prepared-sample.h5 [-o out] [--kallisto] [--num-samples N] [--sample-counts]
        [--transformation polee-transform.h5] [--trim-prefix P] [--seed N] [--transcript-ids ids.txt]
        [--transcript-lengths lens.txt] [--batch B]

The reference names transcripts from --annotations / --sequences; GFF and FASTA parsing is out of scope here (as in
polee_amd.gibbs), so those flags and --exclude-transcripts are not offered: the ids come from a text file with one id per line
(--transcript-ids) and the lengths written to the kallisto file from one with one integer per line (--transcript-lengths).
Without them the ids are 1..n and the lengths -1.  With --transformation the tree AND the ids come from that file (its
transcript_ids), as in main.jl:776-779.  An ids list whose length is not n is an error.  --uniform-gene-prior is parsed and never
used by the reference's handler; it is left out.

One reference quirk is fixed on purpose: the CSV branch computes the default file name and then opens parsed_args["output"]
(main.jl:909-912), which fails without --output; here the CSV goes to the computed name, polee-sample.csv by default.  The counts
of --sample-counts are an exact multinomial draw, not the reference's m binary searches; they are the same
distribution, not the same stream of numbers."""
import argparse
import ctypes as C
import datetime
import sys

import numpy as np

from . import _lib as L
from . import h5io
from ._lib import arr, check, ptr, f32p, f64p, i64p, u32p

DEFAULT_SEED = 123456789
DEFAULT_BATCH = 16
COUNT_EXPECTED, COUNT_SAMPLED = 0, 1


class ApproxSampleStream(L.Handle):
    """A stream of draws from one fitted approximation on the GPU (polee_sampler): t a PolyaTreeTransform, mu / sigma / alpha f32
    [n-1] (sigma = exp(omega)), efflens f32 [n], m reads.  Draw d of a seed is the same whatever the batch sizes."""
    _destroy = "polee_sampler_destroy"

    def __init__(self, t, mu, sigma, alpha, efflens, m, seed=DEFAULT_SEED):
        self.t, self.ctx, self.n, self.m = t, t.ctx, int(t.n), int(m)
        mu, sigma, alpha = (arr(a, np.float32).reshape(-1) for a in (mu, sigma, alpha))
        l = arr(efflens, np.float32).reshape(-1)
        if mu.size != self.n - 1 or sigma.size != self.n - 1 or alpha.size != self.n - 1 or l.size != self.n:
            raise ValueError("mu, sigma, alpha need n - 1 = %d entries and efflens n" % (self.n - 1))
        self._h = C.c_void_p()
        check(L.lib().polee_sampler_create(t._h, ptr(mu, f32p), ptr(sigma, f32p), ptr(alpha, f32p), ptr(l, f32p), C.c_int64(self.m),
                                           C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.byref(self._h)), self.ctx._h)

    @property
    def num_draws(self):
        k = C.c_int64()
        check(L.lib().polee_sampler_num_draws(self._h, C.byref(k)), self.ctx._h)
        return k.value

    def next(self, count, props=True, counts=False, sample_counts=False, raw=False, z0=None):
        """The next `count` draws -> dict with the outputs asked for: props f32 [count, n] (efflen-adjusted, rows sum to 1), counts
        f64 [count, n] (prop_to_counts: expected counts, or sampled ones), raw f32 [count, n] (the draws before the adjustment).
        z0: caller-supplied N(0,1) noise [count, n-1]."""
        count = int(count)
        z = None if z0 is None else arr(z0, np.float32).reshape(count, self.n - 1)
        out = {}
        if raw:
            out["raw"] = np.empty((count, self.n), np.float32)
        if props:
            out["props"] = np.empty((count, self.n), np.float32)
        if counts:
            out["counts"] = np.empty((count, self.n), np.float64)
        check(L.lib().polee_sampler_next(self._h, C.c_int32(count), C.c_int32(COUNT_SAMPLED if sample_counts else COUNT_EXPECTED),
                                         ptr(z, f32p), ptr(out.get("raw"), f32p), ptr(out.get("props"), f32p),
                                         ptr(out.get("counts"), f64p)), self.ctx._h)
        return out

    def mean(self, counts=True, sample_counts=False):
        """(post_mean f32 [n], est_counts f64 [n] or None): the mean of all props so far and prop_to_counts of it."""
        pm = np.empty(self.n, np.float32)
        ec = np.empty(self.n, np.float64) if counts else None
        check(L.lib().polee_sampler_mean(self._h, ptr(pm, f32p), ptr(ec, f64p),
                                         C.c_int32(COUNT_SAMPLED if sample_counts else COUNT_EXPECTED)), self.ctx._h)
        return pm, ec


def multinomial_counts(p, m, seed=DEFAULT_SEED, first_draw=0, ctx=None):
    """Exact multinomial draws of m items on the GPU (polee_multinomial_counts): p [D, n] (or [n]) shares >= 0, not necessarily
    normalised -> u32 counts of the same shape, every row summing to m.  Row r is draw first_draw + r: a pure function of (its
    shares, m, seed, draw index)."""
    from .core import default_context
    ctx = ctx or default_context()
    p = arr(p, np.float64)
    one = p.ndim == 1
    p2 = p.reshape(1, -1) if one else p
    if p2.ndim != 2 or p2.shape[0] < 1 or p2.shape[1] < 1:
        raise ValueError("p must be [D, n] or [n], not empty")
    out = np.empty(p2.shape, np.uint32)
    check(L.lib().polee_multinomial_counts(ctx._h, ptr(p2, f64p), C.c_int32(p2.shape[0]), C.c_int64(p2.shape[1]), C.c_int64(int(m)),
                                           C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(first_draw)), ptr(out, u32p)),
          ctx._h)
    return out[0] if one else out


def debug_binomial(N, p, seed=DEFAULT_SEED, ctx=None):
    """Test hook (polee_debug_binomial): one Binomial(N[i], p[i]) variate per entry -> i64."""
    from .core import default_context
    ctx = ctx or default_context()
    N, p = arr(N, np.int64).reshape(-1), arr(p, np.float64).reshape(-1)
    if N.size != p.size:
        raise ValueError("N and p differ in length")
    out = np.empty(N.size, np.int64)
    check(L.lib().polee_debug_binomial(ctx._h, ptr(N, i64p), ptr(p, f64p), C.c_int64(N.size), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                       ptr(out, i64p)), ctx._h)
    return out


def write_kallisto(output_filename, count_batches, est_counts, efflens, transcript_ids, transcript_lengths, call=""):
    """The kallisto HDF5 layout of main.jl:886-907 for sleuth.  count_batches: an iterable of f64 [B, n] arrays, the counts of
    successive draws -- each batch is written as it arrives (bootstrap/bs0, bs1, ...), the draws are never held together.
    est_counts: f64 [n], or a callable evaluated once the batches are consumed (the posterior mean is known only then).  Returns
    the number of bootstraps written."""
    efflens = np.asarray(efflens, np.float64).reshape(-1)
    n = efflens.size
    ids = [str(t) for t in transcript_ids]
    lens = np.asarray(transcript_lengths, np.int64).reshape(-1)
    if len(ids) != n or lens.size != n:
        raise ValueError("ids / lengths: %d / %d given for %d transcripts" % (len(ids), lens.size, n))
    k = 0
    with h5io.File(output_filename, "w") as f:
        f.create_group("aux")
        f.write("aux/eff_lengths", efflens)
        f.write("aux/lengths", lens)
        f.write_strings("aux/ids", ids)
        f.write_strings("aux/call", [call])
        f.write("aux/index_version", np.array([-1], np.int64))
        f.write_strings("aux/kallisto_version", "polee sample")
        f.write_strings("aux/start_time", datetime.datetime.now().isoformat())
        f.create_group("bootstrap")
        for batch in count_batches:
            batch = np.asarray(batch, np.float64)
            if batch.ndim != 2 or batch.shape[1] != n:
                raise ValueError("a batch of counts must be [B, %d]" % n)
            for row in batch:
                f.write("bootstrap/bs%d" % k, row)
                k += 1
        f.write("aux/num_bootstrap", np.array([k], np.int64))
        ec = est_counts() if callable(est_counts) else est_counts
        ec = np.asarray(ec, np.float64).reshape(-1)
        if ec.size != n:
            raise ValueError("est_counts: %d given for %d transcripts" % (ec.size, n))
        f.write("est_counts", ec)
    return k


def write_csv(output_filename, post_mean, transcript_ids):
    """main.jl:913-916: a header `transcript_id,tpm`, then 1e6 post_mean[j] (Float64 product of the Float32 mean) per transcript."""
    pm = np.asarray(post_mean, np.float32).reshape(-1)
    if len(transcript_ids) != pm.size:
        raise ValueError("ids: %d given for %d transcripts" % (len(transcript_ids), pm.size))
    with open(output_filename, "w") as out:
        out.write("transcript_id,tpm\n")
        for tid, v in zip(transcript_ids, pm.astype(np.float64).tolist()):
            out.write("%s,%r\n" % (tid, 1e6 * v))


def default_output_filename(kallisto):
    return "polee-sample.h5" if kallisto else "polee-sample.csv"


def resolve_names(n, transcript_ids=None, transcript_lengths=None, transformation=None, trim_prefix=None):
    """(ids, lengths) as the handler names them: ids from the transformation file when one is given (main.jl:776-779), else the
    caller's, else 1..n; --trim-prefix removes every occurrence of the prefix string (replace, main.jl:810-815); lengths default -1."""
    if transformation is not None:
        ids = h5io.read_transformation_ids(transformation)
    elif transcript_ids is not None:
        ids = [str(t) for t in transcript_ids]
    else:
        ids = [str(j) for j in range(1, n + 1)]
    if trim_prefix is not None:
        ids = [t.replace(trim_prefix, "") for t in ids]
    if len(ids) != n:
        raise ValueError("Prepared sample has %d transcripts, %d transcript ids were given." % (n, len(ids)))
    lens = np.full(n, -1, np.int64) if transcript_lengths is None else np.asarray(transcript_lengths, np.int64).reshape(-1)
    if lens.size != n:
        raise ValueError("transcript lengths: %d given for %d transcripts" % (lens.size, n))
    return ids, lens


def polee_sample(prepared_sample_filename, output_filename=None, kallisto=False, num_samples=1000, sample_counts=False,
                 transformation=None, trim_prefix=None, seed=DEFAULT_SEED, transcript_ids=None, transcript_lengths=None,
                 batch=DEFAULT_BATCH, ctx=None, call=""):
    """polee_sample (main.jl:756-919) on the GPU: num_samples draws of the prepared sample's approximation, each divided by the
    effective lengths and renormalised; their mean as TPMs to a CSV, or with kallisto=True est_counts and one bootstrap per draw to
    a kallisto-style HDF5.  Returns the posterior mean, f32 [n]."""
    from .core import PolyaTreeTransform, default_context
    if num_samples < 1 or batch < 1:
        raise ValueError("num_samples and batch must be positive")
    ps = h5io.read_prepared_sample(prepared_sample_filename)  # (runs the version check)
    from .core import require_default_approximation
    require_default_approximation(ps, prepared_sample_filename)
    n, m = ps["n"], ps["m"]
    ids, lens = resolve_names(n, transcript_ids, transcript_lengths, transformation, trim_prefix)
    if transformation is not None:
        parents, js = h5io.read_transformation(transformation)
    else:
        parents, js = ps["node_parent_idxs"], ps["node_js"]
        if parents is None or js is None:
            raise ValueError("%s holds no tree: give --transformation" % prepared_sample_filename)
    if output_filename is None:
        output_filename = default_output_filename(kallisto)
    efflens = ps["effective_lengths"]
    t = PolyaTreeTransform(parents, js, ctx=ctx or default_context())
    if t.n != n:
        raise ValueError("the tree has %d leaves, the prepared sample %d transcripts" % (t.n, n))
    stream = ApproxSampleStream(t, ps["mu"], np.exp(ps["omega"]), ps["alpha"], efflens, m, seed)

    def batches(want_counts):
        done = 0
        while done < num_samples:
            k = min(batch, num_samples - done)
            out = stream.next(k, props=False, counts=want_counts, sample_counts=sample_counts)
            done += k
            yield out.get("counts")

    if kallisto:
        write_kallisto(output_filename, batches(True), lambda: stream.mean(True, sample_counts)[1], efflens, ids, lens, call)
    else:
        for _ in batches(False):
            pass
    post_mean = stream.mean(False)[0]
    if not kallisto:
        write_csv(output_filename, post_mean, ids)
    stream.close()
    return post_mean


def _read_lines(filename):
    with open(filename) as f:
        return [line.strip() for line in f if line.strip()]


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    ap = argparse.ArgumentParser(prog="python -m polee_amd.sample", description=__doc__.split("\n\n")[0])
    ap.add_argument("prepared_sample", metavar="prepared-sample.h5")
    ap.add_argument("--output", "-o")
    ap.add_argument("--kallisto", action="store_true", help="Output samples in a format compatible with kallisto, for use with sleuth.")
    ap.add_argument("--num-samples", type=int, default=1000, metavar="N", help="Number of samples to generate.")
    ap.add_argument("--sample-counts", action="store_true",
                    help="Generate integer counts by sampling the reads of every draw instead of expected counts.")
    ap.add_argument("--transformation", metavar="polee-transform.h5", help="Tree (and transcript ids) from this file instead of the sample's.")
    ap.add_argument("--trim-prefix", metavar="P", help="Remove this prefix string from transcript ids.")
    ap.add_argument("--seed", type=int, default=DEFAULT_SEED, metavar="N", help="RNG seed")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (default 1..n).")
    ap.add_argument("--transcript-lengths", metavar="lens.txt", help="Transcript lengths, one per line (default -1).")
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, metavar="B", help="Draws per device batch.")
    a = ap.parse_args(argv)
    ids = _read_lines(a.transcript_ids) if a.transcript_ids else None
    lens = np.array([int(v) for v in _read_lines(a.transcript_lengths)], np.int64) if a.transcript_lengths else None
    from .core import WrongApproximationError
    try:
        polee_sample(a.prepared_sample, a.output, kallisto=a.kallisto, num_samples=a.num_samples, sample_counts=a.sample_counts,
                     transformation=a.transformation, trim_prefix=a.trim_prefix, seed=a.seed, transcript_ids=ids,
                     transcript_lengths=lens, batch=a.batch, call=" ".join(argv))
    except WrongApproximationError as e:
        sys.exit(str(e))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""`polee model tsne` on the GPU (models/tsne.jl, models/polee_tsne.py): parametric t-SNE of transcript expression.

RNASeqTSNE trains the linear embedding z = log(x) W on a fresh draw x from the samples' fitted approximations at every step: the
pairwise distance between the batch samples over all transcripts (the variance of the log-ratio), the t-SNE objective and the Adam step
run on the device (csrc/tsne.hip, polee_tsne_*), no draw visits the host.

    python -m polee_amd.tsne experiment.yml [--num-components N] [--batch-size N] [--posterior-mean] [--output-z tsne-z.csv]

writes the samples' positions (`sample,component1,...`) as write_pca_z (models/tsne.jl:171-188) does.

Where the reference is broken or ill-defined: its sampler call has a stale signature (polee_tsne.py:222-230),
so the intent -- one draw per sample per evaluation -- is what is built; the bias of the embedding has an exactly zero gradient and stays
at zero; --posterior-mean, which the reference parses and never reads, selects the point path (x = the log of the posterior means, no
draws); W0 and the minibatches come from NumPy generators keyed by the seed (initial_weights, minibatches).
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib as L
from ._lib import arr, check, f32p, f64p, i32p, ptr
from ._model import MASK, Handle, approx_of, draw_seed, make_opts, z0_flat
from .core import default_context

NUM_STEPS = 500            # models/polee_tsne.py:355
EMBED_DRAWS = 10           # models/polee_tsne.py:393
TARGET_PERPLEXITY = 50.0   # models/polee_tsne.py:216
BATCH_SIZE = 100           # models/tsne.jl:41-45
DEFAULT_SEED = 123456789


class TSNEOpts(C.Structure):
    """polee_tsne_opts (include/polee_hip.h)"""
    _fields_ = [("num_components", C.c_int32), ("use_vlr", C.c_int32), ("alpha", C.c_float), ("eps", C.c_float),
                ("learning_rate", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float)]


def initial_weights(seed, n, num_components):
    """W0 [n, C] ~ N(0, 1e-4) (polee_tsne.py:298) from default_rng([seed, 0]), cast to f32"""
    return np.random.default_rng([int(seed), 0]).normal(0.0, 1e-4, (int(n), int(num_components))).astype(np.float32)


def minibatches(seed, S, B, count, first=0):
    """batches first .. first + count - 1 of the stream default_rng([seed, 1]): batch i = the first B entries of the i-th successive
    permutation of 0 .. S-1 (polee_tsne.py:366-370); i32 [count, B]"""
    rng = np.random.default_rng([int(seed), 1])
    for _ in range(int(first)):
        rng.permutation(int(S))
    return np.array([rng.permutation(int(S))[:int(B)] for _ in range(int(count))], np.int32).reshape(int(count), int(B))


def find_sigmas(delta, target_perplexity):
    """find_sigmas (polee_tsne.py:64-103) on a distance matrix [S, S], in float64: per row lo = 1e-2, hi = 10 sqrt(max_j delta_ij),
    exactly 20 bisection steps (a step at which every e_j underflows raises lo and counts), the result (lo + hi) / 2; f32 [S]"""
    delta = np.asarray(delta, np.float64)
    S = delta.shape[0]
    sigmas = np.zeros(S, np.float32)
    for i in range(S):
        lo, hi = 1e-2, 10.0 * np.sqrt(delta[i].max())
        for _ in range(20):
            sigma = 0.5 * (lo + hi)
            e = np.exp(-delta[i] / (2.0 * sigma * sigma))
            e[i] = 0.0
            tot = e.sum()
            if tot == 0.0:
                lo = sigma
                continue
            p = e / tot
            p = p[p > 1e-16]
            if 2.0 ** (-(p * np.log2(p)).sum()) > target_perplexity:
                hi = sigma
            else:
                lo = sigma
        sigmas[i] = 0.5 * (lo + hi)
    return sigmas


class RNASeqTSNE(Handle):
    """The embedding of estimate_tsne (models/polee_tsne.py:213-398): W [n, C], zero until set_params.  Every method takes either
    `vars` (LoadedSamples.variables, an RNASeqApproxLikelihood, or the dict of create_tensorflow_variables!: a fresh draw) or `x`
    [S, n] (log expression already: the point path).  Options (num_components, use_vlr, alpha, eps, learning_rate, beta1, beta2,
    epsilon) default to the reference's.  `seed`, `z0` and the explicit batches are additions: the draw with index i uses
    seed + 0x9E3779B97F4A7C15 i, z0 replaces the device's N(0,1) noise."""
    _destroy = "polee_tsne_destroy"

    def __init__(self, n, num_samples, ctx=None, **opts):
        self.n, self.S = int(n), int(num_samples)
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        self.t = 0  # (mirror of the handle's step clock)
        self.opts = make_opts(TSNEOpts, L.lib().polee_tsne_default_opts, opts)
        self.C = int(self.opts.num_components)
        check(L.lib().polee_tsne_create(self.ctx._h, self.n, self.S, C.byref(self.opts), C.byref(self._h)), self.ctx._h)

    # ---- parameters
    def get_params(self):
        """W [n, C]"""
        w = np.empty((self.n, self.C), np.float32)
        check(L.lib().polee_tsne_get_params(self._h, ptr(w, f32p)), self.ctx._h)
        return w

    def set_params(self, w):
        """The Adam moments and the step clock stay as they are (reset() zeroes them)."""
        w = arr(w, np.float32)
        if w.shape != (self.n, self.C):
            raise ValueError("expected W [%d, %d]" % (self.n, self.C))
        check(L.lib().polee_tsne_set_params(self._h, ptr(w, f32p)), self.ctx._h)

    def reset(self):
        check(L.lib().polee_tsne_reset(self._h), self.ctx._h)
        self.t = 0

    def set_sigmas(self, sigmas):
        s = arr(sigmas, np.float32).reshape(-1)
        if s.size != self.S:
            raise ValueError("expected %d bandwidths" % self.S)
        check(L.lib().polee_tsne_set_sigmas(self._h, ptr(s, f32p)), self.ctx._h)

    # ---- argument plumbing
    def _x(self, x):
        x = arr(x, np.float32)
        if x.shape != (self.S, self.n):
            raise ValueError("x must be [%d, %d]" % (self.S, self.n))
        return x

    def _lik(self, vars):
        ap = approx_of(vars, self.ctx)
        if ap.n != self.n or ap.S != self.S:
            raise ValueError("the approximation is [%d, %d], the model [%d, %d]" % (ap.S, ap.n, self.S, self.n))
        return ap

    def _z0(self, z0, draws):
        return z0_flat(z0, draws * self.S * (self.n - 1))

    @staticmethod
    def _batches(batches):
        b = arr(np.atleast_2d(batches), np.int32)
        if b.ndim != 2:
            raise ValueError("batches must be [niter, B]")
        return b

    # ---- the reference's pieces
    def distances(self, vars=None, x=None, seed=DEFAULT_SEED, z0=None):
        """delta f64 [S, S] of one draw (pairwise_vlr, :17-26; pairwise_l2_sq, :42-48, without use_vlr), or of x"""
        delta = np.empty((self.S, self.S), np.float64)
        if x is not None:
            x = self._x(x)
            check(L.lib().polee_tsne_distances_points(self._h, ptr(x, f32p), ptr(delta, f64p)), self.ctx._h)
        else:
            ap = self._lik(vars)
            z = self._z0(z0, 1)
            check(L.lib().polee_tsne_distances(self._h, ap._h, ptr(z, f32p), C.c_uint64(seed & MASK), ptr(delta, f64p)), self.ctx._h)
        return delta

    def find_sigmas(self, vars=None, x=None, target_perplexity=TARGET_PERPLEXITY, seed=DEFAULT_SEED, z0=None):
        """find_sigmas (:64-103, :236-238) on ONE draw of all samples (draw index -1), in float64 on the host from the device's
        distance matrix; the target is min(target_perplexity, S - 1).  Sets and returns the bandwidths f32 [S]."""
        delta = self.distances(vars, x, seed=draw_seed(seed, -1), z0=z0)
        sigmas = find_sigmas(delta, min(float(target_perplexity), float(self.S) - 1.0))
        self.set_sigmas(sigmas)
        return sigmas

    def loss_and_gradient(self, batch, vars=None, x=None, seed=DEFAULT_SEED, z0=None):
        """One evaluation of the loss (:337) on the batch and its gradient, no update: (loss, g_W [n, C]) -- the numbers a fit step
        feeds to Adam."""
        b = arr(batch, np.int32).reshape(-1)
        loss, gw = np.empty(1, np.float32), np.empty((self.n, self.C), np.float32)
        if x is not None:
            x = self._x(x)
            check(L.lib().polee_tsne_eval_points(self._h, ptr(x, f32p), ptr(b, i32p), b.size, ptr(loss, f32p), ptr(gw, f32p)),
                  self.ctx._h)
        else:
            ap = self._lik(vars)
            z = self._z0(z0, 1)
            check(L.lib().polee_tsne_eval(self._h, ap._h, ptr(b, i32p), b.size, ptr(z, f32p), C.c_uint64(seed & MASK), ptr(loss, f32p),
                                          ptr(gw, f32p)), self.ctx._h)
        return float(loss[0]), gw

    def fit(self, niter, vars=None, x=None, batch_size=BATCH_SIZE, seed=DEFAULT_SEED, batches=None, z0=None):
        """niter Adam steps (:355-375); the step clock runs on across calls, so fit(2) then fit(3) equals fit(5).  Step t uses the
        draw with index t - 1 and, unless `batches` [niter, B] are given, batch t - 1 of minibatches(seed, S, min(batch_size, S)).
        Returns the loss trace."""
        niter = int(niter)
        if batches is None:
            batches = minibatches(seed, self.S, min(int(batch_size), self.S), niter, first=self.t)
        b = self._batches(batches)
        if b.shape[0] != niter:
            raise ValueError("%d batches for %d steps" % (b.shape[0], niter))
        trace = np.empty(niter, np.float32)
        if x is not None:
            x = self._x(x)
            check(L.lib().polee_tsne_fit_points(self._h, ptr(x, f32p), ptr(b, i32p), b.shape[1], niter, ptr(trace, f32p)), self.ctx._h)
        else:
            ap = self._lik(vars)
            z = self._z0(z0, niter)
            check(L.lib().polee_tsne_fit(self._h, ap._h, ptr(b, i32p), b.shape[1], niter, C.c_uint64(seed & MASK), ptr(z, f32p),
                                         ptr(trace, f32p)), self.ctx._h)
        self.t += niter
        return trace

    def embed(self, vars=None, x=None, ndraws=EMBED_DRAWS, seed=DEFAULT_SEED, z0=None):
        """The mean of z over ndraws fresh draws (:392-395), draw i under seed + 0x9E3779B97F4A7C15 i; or z of x.  f32 [S, C]"""
        z = np.empty((self.S, self.C), np.float32)
        if x is not None:
            x = self._x(x)
            check(L.lib().polee_tsne_embed_points(self._h, ptr(x, f32p), ptr(z, f32p)), self.ctx._h)
        else:
            ap = self._lik(vars)
            zz = self._z0(z0, int(ndraws))
            check(L.lib().polee_tsne_embed(self._h, ap._h, int(ndraws), C.c_uint64(seed & MASK), ptr(zz, f32p), ptr(z, f32p)),
                  self.ctx._h)
        return z


def estimate_tsne(vars, num_components=2, batch_size=BATCH_SIZE, x0_log=None, use_posterior_mean=False, num_steps=NUM_STEPS,
                  target_perplexity=TARGET_PERPLEXITY, alpha=1.0, use_vlr=True, learning_rate=1e-6, seed=DEFAULT_SEED, ctx=None,
                  return_trace=False):
    """estimate_tsne (models/polee_tsne.py:213-398) as models/tsne.jl:88-94 calls it (use_vlr=True, no neural network): bandwidths
    from one draw, W0 ~ N(0, 1e-4), num_steps Adam steps on minibatches of min(batch_size, S) samples, the mean of z over 10 further
    draws; f32 [S, num_components].  use_posterior_mean: x0_log [S, n] takes the place of every draw."""
    if use_posterior_mean:
        x = np.asarray(x0_log, np.float32)
        S, n = x.shape
        src = dict(x=x)
    else:
        ap = approx_of(vars, ctx)
        S, n = ap.S, ap.n
        src = dict(vars=ap)
    ts = RNASeqTSNE(n, S, ctx=ctx, num_components=int(num_components), use_vlr=int(bool(use_vlr)), alpha=alpha,
                    learning_rate=learning_rate)
    ts.find_sigmas(target_perplexity=target_perplexity, seed=seed, **src)
    ts.set_params(initial_weights(seed, n, num_components))
    trace = ts.fit(num_steps, batch_size=batch_size, seed=seed, **src)
    z = ts.embed(seed=draw_seed(seed, num_steps), **src)
    return (z, trace) if return_trace else z


def parser():
    ap = argparse.ArgumentParser(prog="python -m polee_amd.tsne", description=__doc__.split("\n\n")[0])
    ap.add_argument("experiment", metavar="experiment.yml", help="Experiment specification")
    ap.add_argument("--feature", default="transcript", metavar="F", help="One of transcript, gene, splicing")
    ap.add_argument("--num-components", type=int, default=2, metavar="N", help="Number of t-SNE dimensions")
    ap.add_argument("--posterior-mean", action="store_true", help="Use posterior mean point estimate instead of the full model")
    ap.add_argument("--output-z", default="tsne-z.csv", metavar="filename", help="Output file for t-SNE projection")
    ap.add_argument("--max-num-samples", type=int, default=None, metavar="N",
                    help="Only run the model on a randomly selected subset of N samples")
    ap.add_argument("--batch-size", type=int, default=BATCH_SIZE, metavar="N", help="Sample over mini-batches of size N")
    # (the rest are additions to the reference's interface)
    ap.add_argument("--num-steps", type=int, default=NUM_STEPS, metavar="N", help="Optimiser steps (addition)")
    ap.add_argument("--perplexity", type=float, default=TARGET_PERPLEXITY, metavar="P", help="Target perplexity (addition)")
    ap.add_argument("--learning-rate", type=float, default=1e-6, metavar="LR", help="Adam learning rate (addition)")
    ap.add_argument("--l2", action="store_true", help="Squared Euclidean distance instead of the variance of the log-ratio (addition)")
    ap.add_argument("--seed", type=int, default=DEFAULT_SEED, metavar="N", help="RNG seed (addition)")
    ap.add_argument("--device", type=int, default=0, metavar="D", help="GPU to run on (addition)")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (addition; default 1..n)")
    return ap


def main(argv=None):
    a = parser().parse_args(sys.argv[1:] if argv is None else argv)
    if a.feature not in ("transcript", "gene", "splicing"):
        raise SystemExit("%s is not a supported feature." % a.feature)
    if a.feature in ("splicing", "gene"):
        raise SystemExit("%s feature is not yet implemented." % a.feature)
    if not 1 <= a.num_components <= 16:
        raise SystemExit("--num-components must be 1..16")
    if a.num_steps < 1 or a.batch_size < 2 or not a.perplexity > 0 or not a.learning_rate > 0:
        raise SystemExit("--num-steps, --perplexity and --learning-rate must be positive, --batch-size at least 2")
    from . import estimate, h5io
    from .core import Context
    from .pca import read_experiment, write_pca_z
    from .sample import _read_lines, resolve_names
    spec = read_experiment(a.experiment)
    filenames, _, _ = estimate.read_specification(spec)
    if not filenames:
        raise SystemExit("%s names no samples" % a.experiment)
    n = h5io.read_prepared_sample(filenames[0])["n"]
    if a.transcript_ids:
        resolve_names(n, _read_lines(a.transcript_ids))  # (checked against n; the output names samples only)
    ctx = Context(a.device)
    ls = estimate.load_samples_from_specification(spec, n, max_num_samples=a.max_num_samples, ctx=ctx)
    if len(ls.sample_names) < 2:
        raise SystemExit("t-SNE needs at least two samples")
    z = estimate_tsne(ls.variables, a.num_components, a.batch_size, x0_log=np.log(ls.x0_values), use_posterior_mean=a.posterior_mean,
                      num_steps=a.num_steps, target_perplexity=a.perplexity, use_vlr=not a.l2, learning_rate=a.learning_rate,
                      seed=a.seed, ctx=ctx)
    if a.output_z is not None:
        write_pca_z(a.output_z, ls.sample_names, z)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""`polee model pca` on the GPU (models/pca.jl, models/polee_pca.py:14-92): probabilistic PCA of transcript expression.

RNASeqPCA is the regression model whose design matrix is a latent z [S, C] with a Normal(0, 1) prior and a point surrogate; z is a
device-resident parameter of the regression handle (polee_regression_set_latent_design) and is trained inside the captured step, so a
fit is niter graph replays with no host work between them.

    python -m polee_amd.pca experiment.yml [--num-components N] [--output-z pca-z.csv] [--output-w w.csv]

writes the samples' positions (`sample,component1,...`) and, with --output-w, the transcripts' weights
(`transcript_id,component1,...`), as write_pca_z / write_pca_w (models/pca.jl:179-223) do.
"""
import argparse
import ctypes as C
import math
import sys

import numpy as np

from . import _lib as L
from ._lib import check, f32p, ptr
from .core import RNASeqApproxLikelihood
from .regression import RNASeqLinearRegression, choose_knots, estimate_sample_scales

NUM_STEPS_TRANSCRIPT = 12000  # models/pca.jl:165


class RNASeqPCA(RNASeqLinearRegression):
    """RNASeqPCA (models/polee_pca.py:14-92).  `vars`: the dict of create_tensorflow_variables! (or LoadedSamples.variables, or an
    RNASeqApproxLikelihood); unused with point estimates.  `seed` draws the initial qw_loc = 0.01 N(0, 1) (:50)."""

    def __init__(self, vars, x_init, sample_scales, use_point_estimates, latent_dimensionality=2, kernel_regression_degree=15,
                 kernel_regression_bandwidth=1.0, seed=123456789, ctx=None):
        x_init = np.asarray(x_init, np.float32)
        num_samples, num_features = x_init.shape
        self.latent_dimensionality = int(latent_dimensionality)
        if self.latent_dimensionality < 1:
            raise ValueError("latent_dimensionality must be positive")
        lik = None
        if not use_point_estimates:
            if isinstance(vars, dict) and isinstance(vars.get("approx"), RNASeqApproxLikelihood):
                vars = vars["approx"]
            lik = vars if isinstance(vars, RNASeqApproxLikelihood) else RNASeqApproxLikelihood(vars, ctx=ctx)
        x_init_mean = x_init.astype(np.float64).mean(axis=0)
        deg = int(kernel_regression_degree)
        x_scale_hinges = choose_knots(x_init_mean.min(), x_init_mean.max(), deg)  # (:26-28)
        z0 = np.zeros((num_samples, self.latent_dimensionality), np.float32)  # qz_loc_var (:33)
        # (:44-48: use_distortion = True, scale_penalty = 1e-3)
        super().__init__(z0, x_init, lik, math.log(1.0 / num_features), 12.0, x_scale_hinges, sample_scales, True, 1e-3,
                         use_point_estimates, deg, kernel_regression_bandwidth, ctx=ctx)
        self.set_latent_design(z0, 1.0)
        p = self.get_flat_params()
        rng = np.random.default_rng(seed)
        self.unflatten(p)["qw_loc"][...] = 0.01 * rng.standard_normal((self.latent_dimensionality, num_features))
        self.set_flat_params(p)
        check(L.lib().polee_regression_set_learning_rate(self._h, C.c_float(1e-3)), self.ctx._h)  # (:87)

    def fit(self, niter, seed=123456789, noise=None, return_trace=False):
        """fit (models/polee_pca.py:61-92): returns (qz_loc [S, C], qw_loc [C, n])."""
        z = None if noise is None else np.ascontiguousarray(np.asarray(noise, np.float32).reshape(-1))
        if z is not None and z.size != int(niter) * self.num_noise:
            raise ValueError("noise must hold niter x num_noise values")
        trace = np.empty(int(niter), np.float32)
        check(L.lib().polee_regression_fit(self._h, int(niter), C.c_uint64(seed), ptr(z, f32p), ptr(trace, f32p)), self.ctx._h)
        out = (self.get_design(), self.variables()["qw_loc"])
        return out + (trace,) if return_trace else out


# ---- output (models/pca.jl:179-223)
def _julia_float(v):
    """print(::Float32) of Julia: the shortest digits that round-trip, fixed notation for 1e-4 <= |v| < 1e6, else d.ddde[-]x"""
    v = np.float32(v)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "Inf" if v > 0 else "-Inf"
    if v == 0:
        return "-0.0" if np.signbit(v) else "0.0"
    sci = np.format_float_scientific(v, unique=True, trim="0", exp_digits=1)  # d.ddde+xx
    mant, ex = sci.split("e")
    ex = int(ex)
    if -4 <= ex < 6:
        return np.format_float_positional(v, unique=True, trim="0")
    return "%se%d" % (mant, ex)


def write_pca_z(output_filename, sample_names, z):
    """write_pca_z (models/pca.jl:206-223)"""
    z = np.asarray(z, np.float32)
    if z.shape[0] != len(sample_names):
        raise ValueError("z: %d rows for %d samples" % (z.shape[0], len(sample_names)))
    with open(output_filename, "w") as out:
        out.write("sample" + "".join(",component%d" % (j + 1) for j in range(z.shape[1])) + "\n")
        for name, row in zip(sample_names, z):
            out.write(str(name) + "".join("," + _julia_float(v) for v in row) + "\n")


def write_pca_w(output_filename, feature_names, w, feature_type="transcript_id"):
    """write_pca_w (models/pca.jl:179-203): w [C, n], one row per feature"""
    w = np.asarray(w, np.float32)
    if w.shape[1] != len(feature_names):
        raise ValueError("w: %d columns for %d features" % (w.shape[1], len(feature_names)))
    with open(output_filename, "w") as out:
        out.write(feature_type + "".join(",component%d" % (i + 1) for i in range(w.shape[0])) + "\n")
        for j, name in enumerate(feature_names):
            out.write(str(name) + "".join("," + _julia_float(v) for v in w[:, j]) + "\n")


def read_experiment(filename):
    """The experiment specification: YAML when the yaml module is there, else JSON (a subset of YAML)."""
    with open(filename) as f:
        text = f.read()
    try:
        import yaml
    except ImportError:
        import json
        try:
            return json.loads(text)
        except ValueError as e:
            raise SystemExit("%s: the yaml module is not installed, so the experiment file must be JSON (a subset of YAML): %s"
                             % (filename, e))
    return yaml.safe_load(text)


def parser():
    ap = argparse.ArgumentParser(prog="python -m polee_amd.pca", description=__doc__.split("\n\n")[0])
    ap.add_argument("experiment", metavar="experiment.yml", help="Experiment specification")
    ap.add_argument("--feature", default="transcript", metavar="F", help="transcript (isoform is not built)")
    ap.add_argument("--num-components", type=int, default=2, metavar="N", help="Number of PCA components")
    ap.add_argument("--point-estimates", default=None, metavar="KEY",
                    help="Point estimates from the files the experiment names (not built: the class supports them, the loader is missing)")
    ap.add_argument("--output-z", default="pca-z.csv", metavar="filename", help="Output file for PCA projection")
    ap.add_argument("--output-w", default=None, metavar="filename", help="Output file for PCA transcript weights")
    ap.add_argument("--num-steps", type=int, default=NUM_STEPS_TRANSCRIPT, metavar="N", help="Optimiser steps")
    ap.add_argument("--seed", type=int, default=123456789, metavar="N", help="RNG seed")
    ap.add_argument("--device", type=int, default=0, metavar="D", help="GPU to run on")
    ap.add_argument("--max-num-samples", type=int, default=None, metavar="N", help="Use a random subset of the samples")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (default 1..n).")
    return ap


def main(argv=None):
    a = parser().parse_args(sys.argv[1:] if argv is None else argv)
    if a.feature == "isoform":
        raise SystemExit("--feature isoform is not built (RNASeqIsoformPCA's gene latent has 20 dimensions, above the kernel's 16)")
    if a.feature != "transcript":
        raise SystemExit("%s is not a supported feature." % a.feature)
    if a.point_estimates is not None:
        raise SystemExit("--point-estimates is not built: the point-estimate file loader is missing "
                         "(RNASeqPCA itself supports use_point_estimates=True)")
    if not 1 <= a.num_components <= 16:
        raise SystemExit("--num-components must be 1..16")
    spec = read_experiment(a.experiment)
    from . import estimate, h5io
    from .core import Context
    from .sample import _read_lines, resolve_names
    filenames, _, _ = estimate.read_specification(spec)
    if not filenames:
        raise SystemExit("%s names no samples" % a.experiment)
    n = h5io.read_prepared_sample(filenames[0])["n"]
    ids, _ = resolve_names(n, _read_lines(a.transcript_ids) if a.transcript_ids else None)
    ctx = Context(a.device)
    ls = estimate.load_samples_from_specification(spec, n, max_num_samples=a.max_num_samples, ctx=ctx)
    x0_log = np.log(ls.x0_values)
    sample_scales = estimate_sample_scales(x0_log, upper_quantile=0.9)
    pca = RNASeqPCA(ls.variables, x0_log, sample_scales, False, latent_dimensionality=a.num_components, seed=a.seed, ctx=ctx)
    z, w = pca.fit(a.num_steps, seed=a.seed)
    if a.output_w is not None:
        write_pca_w(a.output_w, ids, w)
    if a.output_z is not None:
        write_pca_z(a.output_z, ls.sample_names, z)
    return 0


if __name__ == "__main__":
    sys.exit(main())

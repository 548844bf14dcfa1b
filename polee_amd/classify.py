"""`polee model classify` on the GPU (models/classify.jl, models/polee_classify.py): a multinomial logistic regression on log expression.

RNASeqLogisticRegression is trained on fresh draws from the training samples' fitted approximations at every step and predicts by the
mean class probability over draws from the testing samples' approximations; the draws are made and consumed on the device
(csrc/classify.hip, polee_classify_*), none of them visits the host.

    python -m polee_amd.classify training.yml testing.yml factor [--point-estimates KEY | --kallisto] [--pseudocount C]

writes the testing samples' class probabilities (--output-predictions, `y-predicted.csv`), their true classes one-hot (--output-truth,
`y-true.csv`) and the trained weights (--output-w, `w.csv`, tab-separated) as models/classify.jl:245-254 does.
"""
import argparse
import ctypes as C
import sys

import numpy as np

from . import _lib as L
from ._lib import arr, check, f32p, ptr
from ._model import MASK, Handle, approx_of, draw_seed, make_opts, z0_flat
from .core import default_context

NUM_STEPS = 5000         # models/classify.jl:203-205, :237-239
TESTING_SAMPLES = 100    # models/classify.jl:241-242 (the --testing-samples default of 20 is never read there)
DEFAULT_SEED = 123456789


class ClassifyOpts(C.Structure):
    """polee_classify_opts (include/polee_hip.h)"""
    _fields_ = [("draws_per_step", C.c_int32), ("learning_rate", C.c_float), ("l1_penalty", C.c_float), ("loss_scale", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float)]


class RNASeqLogisticRegression(Handle):
    """RNASeqLogisticRegression (models/polee_classify.py:13-114): w [n, k], x_bias [n], z_bias [k], all zero at first and all trained.
    `vars`: LoadedSamples.variables (its "approx" handle is used), an RNASeqApproxLikelihood, or the dict of
    create_tensorflow_variables!.  Options (draws_per_step, learning_rate, l1_penalty, loss_scale, beta1, beta2, epsilon) default
    to the reference's: 5 draws per step, Adam(1e-4), penalty 0.001.  `seed`, `z0` and `return_trace` are additions: draw i of a
    call uses seed + 0x9E3779B97F4A7C15 i (the bias draw of fit_sample: index -1), z0 replaces the device's N(0,1) noise."""
    _destroy = "polee_classify_destroy"

    def __init__(self, k, n, ctx=None, **opts):
        self.k, self.n = int(k), int(n)
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        self.opts = make_opts(ClassifyOpts, L.lib().polee_classify_default_opts, opts)
        check(L.lib().polee_classify_create(self.ctx._h, self.n, self.k, C.byref(self.opts), C.byref(self._h)), self.ctx._h)

    # ---- parameters
    def get_params(self):
        """(w [n, k], x_bias [n], z_bias [k])"""
        w, xb, zb = np.empty((self.n, self.k), np.float32), np.empty(self.n, np.float32), np.empty(self.k, np.float32)
        check(L.lib().polee_classify_get_params(self._h, ptr(w, f32p), ptr(xb, f32p), ptr(zb, f32p)), self.ctx._h)
        return w, xb, zb

    def set_params(self, w, x_bias, z_bias):
        """The Adam moments and the step clock stay as they are (reset() zeroes them)."""
        w, xb, zb = arr(w, np.float32), arr(x_bias, np.float32).reshape(-1), arr(z_bias, np.float32).reshape(-1)
        if w.shape != (self.n, self.k) or xb.size != self.n or zb.size != self.k:
            raise ValueError("expected w [%d, %d], x_bias [%d], z_bias [%d]" % (self.n, self.k, self.n, self.k))
        check(L.lib().polee_classify_set_params(self._h, ptr(w, f32p), ptr(xb, f32p), ptr(zb, f32p)), self.ctx._h)

    def reset(self):
        check(L.lib().polee_classify_reset(self._h), self.ctx._h)

    def _set_opts(self, **kw):
        for name, v in kw.items():
            setattr(self.opts, name, v)
        check(L.lib().polee_classify_set_opts(self._h, C.byref(self.opts)), self.ctx._h)

    # ---- argument plumbing
    def _labels(self, z_true, S):
        y = arr(np.atleast_2d(z_true), np.float32)
        if y.shape != (S, self.k):
            raise ValueError("z_true must be [%d, %d]" % (S, self.k))
        return y

    def _x(self, x):
        x = arr(np.atleast_2d(x), np.float32)
        if x.shape[1] != self.n:
            raise ValueError("x must be [S, %d]" % self.n)
        return x

    def _lik(self, num_samples, n, vars):
        ap = approx_of(vars, self.ctx)
        if int(n) != self.n or ap.n != self.n or ap.S != int(num_samples):
            raise ValueError("the approximation is [%d, %d], the call says [%d, %d], the classifier has n = %d"
                             % (ap.S, ap.n, num_samples, n, self.n))
        return ap

    # ---- the reference's methods
    def init_bias_sample(self, num_samples, n, vars, seed=DEFAULT_SEED, z0=None):
        """x_bias <- the column mean of the log of one draw (:52-55)"""
        ap = self._lik(num_samples, n, vars)
        z = z0_flat(z0, ap.S * (ap.n - 1))
        check(L.lib().polee_classify_init_bias(self._h, ap._h, ptr(z, f32p), C.c_uint64(seed & MASK)), self.ctx._h)

    def init_bias(self, x):
        """x_bias <- the column mean of x (:75)"""
        x = self._x(x)
        check(L.lib().polee_classify_init_bias_points(self._h, ptr(x, f32p), x.shape[0]), self.ctx._h)

    def loss_and_gradients(self, num_samples=None, n=None, vars=None, z_true=None, x=None, seed=DEFAULT_SEED, z0=None):
        """One evaluation of loss_sample (:43-49; with x: loss, :22-41) and its gradient, no update:
        (loss, g_w [n, k], g_x_bias [n], g_z_bias [k]) -- the numbers a fit step feeds to Adam."""
        loss = np.empty(1, np.float32)
        gw, gxb, gzb = np.empty((self.n, self.k), np.float32), np.empty(self.n, np.float32), np.empty(self.k, np.float32)
        if x is not None:
            x = self._x(x)
            y = self._labels(z_true, x.shape[0])
            check(L.lib().polee_classify_eval_points(self._h, ptr(x, f32p), x.shape[0], ptr(y, f32p), ptr(loss, f32p), ptr(gw, f32p),
                                                     ptr(gxb, f32p), ptr(gzb, f32p)), self.ctx._h)
        else:
            ap = self._lik(num_samples, n, vars)
            y = self._labels(z_true, ap.S)
            z = z0_flat(z0, self.opts.draws_per_step * ap.S * (ap.n - 1))
            check(L.lib().polee_classify_eval(self._h, ap._h, ptr(y, f32p), ptr(z, f32p), C.c_uint64(seed & MASK), ptr(loss, f32p),
                                              ptr(gw, f32p), ptr(gxb, f32p), ptr(gzb, f32p)), self.ctx._h)
        return float(loss[0]), gw, gxb, gzb

    def fit_steps_sample(self, num_samples, n, vars, z_true, niter, seed=DEFAULT_SEED, z0=None):
        """niter Adam steps without the bias initialisation; the step clock runs on across calls.  Returns the loss trace."""
        ap = self._lik(num_samples, n, vars)
        y = self._labels(z_true, ap.S)
        z = z0_flat(z0, int(niter) * self.opts.draws_per_step * ap.S * (ap.n - 1))
        trace = np.empty(int(niter), np.float32)
        check(L.lib().polee_classify_fit(self._h, ap._h, ptr(y, f32p), int(niter), C.c_uint64(seed & MASK), ptr(z, f32p),
                                         ptr(trace, f32p)), self.ctx._h)
        return trace

    def fit_steps(self, x, z_true, niter):
        x = self._x(x)
        y = self._labels(z_true, x.shape[0])
        trace = np.empty(int(niter), np.float32)
        check(L.lib().polee_classify_fit_points(self._h, ptr(x, f32p), x.shape[0], ptr(y, f32p), int(niter), ptr(trace, f32p)),
              self.ctx._h)
        return trace

    def fit_sample(self, num_samples, n, vars, z_true, niter, samples_per_iter=None, seed=DEFAULT_SEED, z0=None, return_trace=False):
        """fit_sample (:51-72): x_bias from one draw, then niter steps of a fresh Adam; returns w [n, k].  samples_per_iter: None
        keeps the handle's draws_per_step (5 unless the constructor was given another, the reference's default); a number becomes
        the handle's option from this call on.  z0 (optional): [niter, draws per step, S, n-1] for the steps; the bias draw keeps
        the device's noise."""
        if samples_per_iter is not None:
            self._set_opts(draws_per_step=int(samples_per_iter))
        self.init_bias_sample(num_samples, n, vars, seed=draw_seed(seed, -1))
        self.reset()
        trace = self.fit_steps_sample(num_samples, n, vars, z_true, niter, seed=seed, z0=z0)
        w = self.get_params()[0]
        return (w, trace) if return_trace else w

    def fit(self, x, z_true, niter, loss_scale=None, return_trace=False):
        """fit (:74-95): x_bias <- the column mean of x, then niter steps of a fresh Adam; returns w [n, k].  loss_scale: None keeps
        the handle's (1 unless the constructor was given another, the reference's default); a number becomes the handle's option
        from this call on."""
        if loss_scale is not None:
            self._set_opts(loss_scale=float(loss_scale))
        self.init_bias(x)
        self.reset()
        trace = self.fit_steps(x, z_true, niter)
        w = self.get_params()[0]
        return (w, trace) if return_trace else w

    def predict_sample(self, num_samples, n, vars, niter, seed=DEFAULT_SEED, z0=None):
        """predict_sample (:105-111): the mean over niter draws of softmax(logits), [S, k]"""
        ap = self._lik(num_samples, n, vars)
        z = z0_flat(z0, int(niter) * ap.S * (ap.n - 1))
        probs = np.empty((ap.S, self.k), np.float32)
        check(L.lib().polee_classify_predict(self._h, ap._h, int(niter), C.c_uint64(seed & MASK), ptr(z, f32p), ptr(probs, f32p)),
              self.ctx._h)
        return probs

    def predict(self, x):
        """predict (:113-114)"""
        x = self._x(x)
        probs = np.empty((x.shape[0], self.k), np.float32)
        check(L.lib().polee_classify_predict_points(self._h, ptr(x, f32p), x.shape[0], ptr(probs, f32p)), self.ctx._h)
        return probs

    def eval_sample(self, num_samples, n, vars, seed=DEFAULT_SEED, z0=None):
        """eval_sample (:97-99): softmax(logits) of one draw"""
        return self.predict_sample(num_samples, n, vars, 1, seed=seed, z0=z0)

    def eval(self, x):
        """eval (:101-103)"""
        return self.predict(x)


# ---- classes and output (models/classify.jl:278-346)
def build_factor_matrix(num_samples, sample_factors, factor, factor_idx=None):
    """build_factor_matrix (models/classify.jl:278-308): (F [num_samples, classes] one-hot f32, factor_idx {option: column}).  The
    reference numbers the options in the iteration order of a Julia Set, which is arbitrary; here the classes are the options in
    SORTED order.  A sample without the factor has the option "missing" (string(missing), :282).  With a given factor_idx (the
    testing set) a sample whose option was not seen in training gets an all-zero row, as in the reference (:302-304)."""
    options = [str(f.get(factor, "missing")) for f in sample_factors]
    if len(options) != int(num_samples):
        raise ValueError("%d samples, %d factor dictionaries" % (num_samples, len(options)))
    if factor_idx is None:
        factor_idx = {opt: i for i, opt in enumerate(sorted(set(options)))}
    F = np.zeros((int(num_samples), len(factor_idx)), np.float32)
    for i, opt in enumerate(options):
        if opt in factor_idx:
            F[i, factor_idx[opt]] = 1.0
    return F, factor_idx


def factor_names_of(factor_idx):
    """models/classify.jl:187-191"""
    names = [None] * len(factor_idx)
    for k, v in factor_idx.items():
        names[v] = k
    return names


def _write_matrix(filename, factor_names, y):
    from .pca import _julia_float
    y = np.asarray(y, np.float32)
    if y.ndim != 2 or y.shape[1] != len(factor_names):
        raise ValueError("%d columns for %d classes" % (y.shape[-1], len(factor_names)))
    with open(filename, "w") as out:
        out.write(",".join(str(f) for f in factor_names) + "\n")
        for row in y:
            out.write(",".join(_julia_float(v) for v in row) + "\n")


def write_classification_probs(factor_names, y_predicted_filename, y_true_filename, y_predicted, y_true):
    """write_classification_probs (models/classify.jl:311-346): a header of class names, then one row per testing sample; values as
    Julia prints Float32"""
    _write_matrix(y_true_filename, factor_names, y_true)
    _write_matrix(y_predicted_filename, factor_names, y_predicted)


def write_w(filename, w):
    """writedlm(output, w) (models/classify.jl:245-247): w [n, k], tab-separated"""
    from .pca import _julia_float
    with open(filename, "w") as out:
        for row in np.asarray(w, np.float32):
            out.write("\t".join(_julia_float(v) for v in row) + "\n")


# ---- point estimates (src/estimate.jl:268-316, models/kallisto.jl:2-26)
def load_point_estimates(filenames, transcript_ids):
    """load_point_estimates (src/estimate.jl:268-316): `transcript_id,tpm` CSVs -> x0 f32 [S, n] = TPM / 1e6; ids the annotation does
    not know are skipped, transcripts a file does not name stay 0."""
    idx = {str(t): j for j, t in enumerate(transcript_ids)}
    x0 = np.zeros((len(filenames), len(idx)), np.float32)
    for i, filename in enumerate(filenames):
        with open(filename) as f:
            header = f.readline().rstrip("\n").split(",")
            if header[:2] != ["transcript_id", "tpm"]:
                raise ValueError("%s: the header must be transcript_id,tpm" % filename)
            for line in f:
                row = line.rstrip("\n").split(",")
                j = idx.get(row[0])
                if j is not None:
                    x0[i, j] = np.float32(float(row[1]) / np.float32(1e6))
    return x0


def counts_to_feature_log_props(xs, efflens, pseudocount):
    """counts_to_feature_log_props! (models/kallisto.jl:2-10) with the identity feature matrix: Float32 counts / effective lengths,
    normalised, + pseudocount / 1e6, log; [1, n]"""
    xs = (np.asarray(xs, np.float32).reshape(-1) / np.asarray(efflens).reshape(-1)).astype(np.float32)  # (xs ./= efflens: stays Float32)
    xs = xs / xs.sum()
    xs = (xs + pseudocount / np.float32(1e6)).astype(np.float32)
    with np.errstate(divide="ignore"):
        return np.log(xs).astype(np.float32).reshape(1, -1)


def read_kallisto_estimates(filenames, pseudocount=0.0):
    """read_kallisto_estimates (models/kallisto.jl:13-26): est_counts and aux/eff_lengths of every file -> log proportions [S, n]"""
    from . import h5io
    rows = []
    for filename in filenames:
        with h5io.File(filename) as f:
            efflens = f.read("aux/eff_lengths", np.float64)
            xs = f.read("est_counts", np.float64).astype(np.float32)
        rows.append(counts_to_feature_log_props(xs, efflens, pseudocount))
    return np.concatenate(rows, axis=0)


def log_point_estimates(x0, pseudocount=None):
    """models/classify.jl:141-147: x0 += pseudocount / 1e6 when one is given, then log (log 0 = -inf without one)"""
    x0 = np.asarray(x0, np.float32)
    if pseudocount is not None:
        x0 = x0 + np.float32(pseudocount / np.float32(1e6))
    with np.errstate(divide="ignore"):
        return np.log(x0).astype(np.float32)


def parser():
    ap = argparse.ArgumentParser(prog="python -m polee_amd.classify", description=__doc__.split("\n\n")[0])
    ap.add_argument("training_experiment", metavar="training.yml", help="Training experiment specification")
    ap.add_argument("testing_experiment", metavar="testing.yml", help="Testing experiment specification")
    ap.add_argument("factor", help="Factor to classify by")
    ap.add_argument("--feature", default="transcript", metavar="F", help="transcript (gene and splicing are not built)")
    ap.add_argument("--point-estimates", default=None, metavar="KEY",
                    help="Use point estimates (transcript_id,tpm CSVs) the experiments name under this key; needs --transcript-ids")
    ap.add_argument("--kallisto", action="store_true", help="Use kallisto maximum likelihood estimates (the samples' `kallisto` key)")
    ap.add_argument("--kallisto-bootstrap", action="store_true", help="(not built)")
    ap.add_argument("--pseudocount", type=float, default=None, metavar="C", help="With a point mode, add C tpm to each value")
    ap.add_argument("--output-predictions", default="y-predicted.csv", metavar="filename", help="Output prediction probability matrix")
    ap.add_argument("--output-truth", default="y-true.csv", metavar="filename", help="Output true classes of the testing samples")
    ap.add_argument("--output-w", default="w.csv", metavar="filename", help="Output trained weights, tab-separated")
    ap.add_argument("--num-steps", type=int, default=NUM_STEPS, metavar="N", help="Optimiser steps")
    ap.add_argument("--testing-samples", type=int, default=TESTING_SAMPLES, metavar="N", help="Classify by averaging over N draws")
    ap.add_argument("--draws-per-step", type=int, default=5, metavar="N", help="Draws per training step")
    ap.add_argument("--learning-rate", type=float, default=1e-4, metavar="LR", help="Adam learning rate")
    ap.add_argument("--seed", type=int, default=DEFAULT_SEED, metavar="N", help="RNG seed")
    ap.add_argument("--device", type=int, default=0, metavar="D", help="GPU to run on")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (default 1..n)")
    return ap


def main(argv=None):
    a = parser().parse_args(sys.argv[1:] if argv is None else argv)
    if a.feature != "transcript":
        raise SystemExit("--feature %s is not built: only transcript" % a.feature)
    if a.kallisto and a.kallisto_bootstrap:
        raise SystemExit("Only one of '--kallisto' and '--kallisto-bootstrap' can be used.")
    if a.kallisto_bootstrap:
        raise SystemExit("--kallisto-bootstrap is not built (the reference marks it TODO and fails on an undefined variable)")
    if a.kallisto and a.point_estimates is not None:
        raise SystemExit("'--point-estimates' is not compatible with '--kallisto'")
    point = a.kallisto or a.point_estimates is not None
    if a.pseudocount is not None and not point:
        raise SystemExit("--pseudocount argument only valid with --point-estimates or --kallisto")
    if a.point_estimates is not None and not a.transcript_ids:
        raise SystemExit("--point-estimates needs --transcript-ids: the CSV rows are matched by transcript id")
    if a.num_steps < 1 or a.testing_samples < 1 or a.draws_per_step < 1:
        raise SystemExit("--num-steps, --testing-samples and --draws-per-step must be positive")
    from . import estimate, h5io
    from .core import Context
    from .pca import read_experiment
    from .sample import _read_lines
    training_spec, testing_spec = read_experiment(a.training_experiment), read_experiment(a.testing_experiment)
    for spec, name in ((training_spec, a.training_experiment), (testing_spec, a.testing_experiment)):
        if not spec.get("samples"):
            raise SystemExit("%s names no samples" % name)
    ctx = Context(a.device)
    if a.kallisto:
        _, _, f_train = estimate.read_specification(training_spec)
        _, _, f_test = estimate.read_specification(testing_spec)
        pc = 0.0 if a.pseudocount is None else a.pseudocount
        x_train = read_kallisto_estimates([s["kallisto"] for s in training_spec["samples"]], pc)
        x_test = read_kallisto_estimates([s["kallisto"] for s in testing_spec["samples"]], pc)
    elif point:
        ids = _read_lines(a.transcript_ids)
        fn_train, _, f_train = estimate.read_specification(training_spec, point_estimates_key=a.point_estimates)
        fn_test, _, f_test = estimate.read_specification(testing_spec, point_estimates_key=a.point_estimates)
        x_train = log_point_estimates(load_point_estimates(fn_train, ids), a.pseudocount)
        x_test = log_point_estimates(load_point_estimates(fn_test, ids), a.pseudocount)
    else:
        filenames, _, _ = estimate.read_specification(training_spec)
        with h5io.File(filenames[0]) as f:  # (n alone: the loader reads the samples)
            n = int(f.read("n", np.int64)[0])
        ls_train = estimate.load_samples_from_specification(training_spec, n, ctx=ctx)
        ls_test = estimate.load_samples_from_specification(testing_spec, n, ctx=ctx)
        f_train, f_test = ls_train.sample_factors, ls_test.sample_factors
    y_train, factor_idx = build_factor_matrix(len(f_train), f_train, a.factor)
    y_test, _ = build_factor_matrix(len(f_test), f_test, a.factor, factor_idx)
    k = len(factor_idx)
    if not 2 <= k <= 16:
        raise SystemExit("factor %s has %d classes in the training set; 2..16 are supported" % (a.factor, k))
    try:
        if point:
            clf = RNASeqLogisticRegression(k, x_train.shape[1], ctx=ctx, learning_rate=a.learning_rate)
            w = clf.fit(x_train, y_train, a.num_steps)
            y_predicted = clf.predict(x_test)
        else:
            clf = RNASeqLogisticRegression(k, n, ctx=ctx, learning_rate=a.learning_rate)
            w = clf.fit_sample(len(f_train), n, ls_train.variables, y_train, a.num_steps, samples_per_iter=a.draws_per_step, seed=a.seed)
            y_predicted = clf.predict_sample(len(f_test), n, ls_test.variables, a.testing_samples, seed=a.seed + 1)
    except L.NonFiniteError as e:
        raise SystemExit("%s\n(a point estimate of 0 has log -inf: give --pseudocount C)" % e)
    write_w(a.output_w, w)
    write_classification_probs(factor_names_of(factor_idx), a.output_predictions, a.output_truth, y_predicted, y_test)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""`polee model random-forest` (models/random-forest.jl): a classification forest on log expression, trained on draws from the training
samples' fitted approximations and predicting by the votes over draws from the testing samples' approximations; forests grown on the
GPU (csrc/forest.hip), or on the host with --host (csrc/forest_host.cpp).  DESIGN.md section 3.14.

    python -m polee_amd.random_forest training.yml testing.yml factor

The forest is this project's own exact definition, not DecisionTree.jl's: the same seed gives the same forest bit for bit from the
device builder, the host builder and the NumPy restatement of the tests.  Training draws use --seed, the forest --seed + 1, testing
draws --seed + 2."""
import argparse
import ctypes as C
import math
import sys

import numpy as np

from . import _lib as L
from ._lib import arr, check, f32p, f64p, i32p, i64p, ptr
from ._model import MASK, Handle, approx_of, make_opts, z0_flat

DEFAULT_SEED = 12345       # models/random-forest.jl:84-87
FOREST_MAX_ROWS = 8192     # POLEE_FOREST_MAX_ROWS (include/polee_hip.h)


class ForestOpts(C.Structure):
    """polee_forest_opts (include/polee_hip.h)"""
    _fields_ = [("ntrees", C.c_int32), ("max_depth", C.c_int32), ("min_samples_leaf", C.c_int32), ("min_samples_split", C.c_int32),
                ("nsubfeatures", C.c_double), ("partial_sampling", C.c_double)]


def _bind():
    lib = L.lib()
    if getattr(lib, "_forest_bound", False):
        return lib
    vp = C.c_void_p
    lib.polee_forest_default_opts.restype = None
    lib.polee_forest_default_opts.argtypes = [C.POINTER(ForestOpts)]
    lib.polee_forest_create.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(ForestOpts), C.POINTER(vp)]
    lib.polee_forest_fit_points.argtypes = [vp, f32p, i32p, C.c_int32, C.c_uint64]
    lib.polee_forest_fit.argtypes = [vp, vp, i32p, C.c_int32, C.c_uint64, C.c_uint64, f32p]
    lib.polee_forest_node_count.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.polee_forest_get_nodes.argtypes = [vp, i64p, i32p, f64p, i32p, i32p, i32p]
    lib.polee_forest_set_nodes.argtypes = [vp, C.c_int32, i64p, i32p, f64p, i32p, i32p, i32p]
    lib.polee_forest_predict_points.argtypes = [vp, f32p, C.c_int32, i32p]
    lib.polee_forest_predict.argtypes = [vp, vp, C.c_int32, C.c_uint64, f32p, i32p]
    lib.polee_forest_log_draws.argtypes = [vp, C.c_int32, C.c_uint64, f32p, f32p]
    lib.polee_forest_build_host.argtypes = [f32p, i32p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(ForestOpts), C.c_uint64, C.c_int64,
                                            C.POINTER(C.c_int64), i64p, i32p, f64p, i32p, i32p, i32p]
    lib.polee_forest_votes_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, i64p, i32p, f64p, i32p, i32p, i32p, f32p, C.c_int32, i32p]
    lib._forest_bound = True
    return lib


def forest_opts(**kw):
    """the reference's defaults (200 trees, 10 sqrt(n) candidate features, full bootstrap), overridden by keyword"""
    return make_opts(ForestOpts, _bind().polee_forest_default_opts, kw)


def _node_arrays(nodes):
    off, feature, threshold, left, right, label = nodes
    return (arr(off, np.int64), arr(feature, np.int32), arr(threshold, np.float64), arr(left, np.int32), arr(right, np.int32),
            arr(label, np.int32))


def build_forest_host(x, labels, k, seed=DEFAULT_SEED, **opts):
    """The forest on the host, no GPU: (tree_off i64 [ntrees+1], feature, threshold f64, left, right, label)."""
    lib = _bind()
    x, labels = arr(np.atleast_2d(x), np.float32), arr(labels, np.int32).reshape(-1)
    N, n = x.shape
    if labels.size != N:
        raise ValueError("%d rows, %d labels" % (N, labels.size))
    o = forest_opts(**opts)
    nb = max(1, int(math.floor(o.partial_sampling * N)))
    cap = o.ntrees * (2 * min(nb, FOREST_MAX_ROWS) - 1)
    off = np.zeros(o.ntrees + 1, np.int64)
    feature, left, right, label = (np.zeros(cap, np.int32) for _ in range(4))
    threshold = np.zeros(cap, np.float64)
    nn = C.c_int64()
    check(lib.polee_forest_build_host(ptr(x, f32p), ptr(labels, i32p), N, n, int(k), C.byref(o), C.c_uint64(seed & MASK), cap, C.byref(nn),
                                      ptr(off, i64p), ptr(feature, i32p), ptr(threshold, f64p), ptr(left, i32p), ptr(right, i32p),
                                      ptr(label, i32p)))
    c = nn.value
    return off, feature[:c].copy(), threshold[:c].copy(), left[:c].copy(), right[:c].copy(), label[:c].copy()


def forest_votes_host(nodes, x, k):
    """votes i32 [R, k] of the forest `nodes` on x [R, n], on the host"""
    lib = _bind()
    off, feature, threshold, left, right, label = _node_arrays(nodes)
    x = arr(np.atleast_2d(x), np.float32)
    votes = np.zeros((x.shape[0], int(k)), np.int32)
    check(lib.polee_forest_votes_host(x.shape[1], int(k), off.size - 1, ptr(off, i64p), ptr(feature, i32p), ptr(threshold, f64p),
                                      ptr(left, i32p), ptr(right, i32p), ptr(label, i32p), ptr(x, f32p), x.shape[0], ptr(votes, i32p)))
    return votes


def log_draws(ap, ndraws, seed=DEFAULT_SEED, z0=None):
    """f32 [ndraws S, n]: the rows fit_sample trains on and predict_sample walks (row d S + s = the device's log of draw d of sample s)"""
    lib = _bind()
    z = z0_flat(z0, ndraws * ap.S * (ap.n - 1))
    out = np.empty((ndraws * ap.S, ap.n), np.float32)
    check(lib.polee_forest_log_draws(ap._h, int(ndraws), C.c_uint64(seed & MASK), ptr(z, f32p), ptr(out, f32p)), ap.ctx._h)
    return out


class RNASeqRandomForest(Handle):
    """A forest of k classes on n features.  Options: ntrees, nsubfeatures, partial_sampling, max_depth, min_samples_leaf,
    min_samples_split.  host=True builds and predicts on the host and takes points only (no GPU, no context).
    Labels are class numbers 0 .. k-1, or one-hot rows [S, k]."""
    _destroy = "polee_forest_destroy"

    def __init__(self, k, n, ctx=None, host=False, **opts):
        self.k, self.n, self.host = int(k), int(n), bool(host)
        self._opts_kw = dict(opts)
        self.opts = forest_opts(**opts)
        self._nodes = None
        self._h = C.c_void_p()
        self.ctx = None
        if not self.host:
            from .core import default_context
            self.ctx = ctx or default_context()
            check(_bind().polee_forest_create(self.ctx._h, self.n, self.k, C.byref(self.opts), C.byref(self._h)), self.ctx._h)
        elif not 2 <= self.k <= 16:
            raise ValueError("2..16 classes are supported")

    def _labels(self, y, S):
        y = np.asarray(y)
        if y.ndim == 2:
            if y.shape != (S, self.k) or not ((y == 0) | (y == 1)).all() or not (y.sum(axis=1) == 1).all():
                raise ValueError("labels must be one-hot [%d, %d]" % (S, self.k))
            y = y.argmax(axis=1)
        y = arr(y, np.int32).reshape(-1)
        if y.size != S:
            raise ValueError("%d labels for %d rows" % (y.size, S))
        return y

    def _x(self, x):
        x = arr(np.atleast_2d(x), np.float32)
        if x.shape[1] != self.n:
            raise ValueError("x must be [rows, %d]" % self.n)
        return x

    def _lik(self, vars):
        ap = approx_of(vars, self.ctx)
        if ap.n != self.n:
            raise ValueError("the approximation has n = %d, the forest n = %d" % (ap.n, self.n))
        return ap

    # ---- the forest
    def nodes(self):
        """(tree_off i64 [ntrees+1], feature i32, threshold f64, left i32, right i32, label i32)"""
        if self.host:
            if self._nodes is None:
                raise ValueError("no forest yet")
            return self._nodes
        lib = _bind()
        nt, nn = C.c_int32(), C.c_int64()
        check(lib.polee_forest_node_count(self._h, C.byref(nt), C.byref(nn)), self.ctx._h)
        off = np.zeros(nt.value + 1, np.int64)
        feature, left, right, label = (np.zeros(nn.value, np.int32) for _ in range(4))
        threshold = np.zeros(nn.value, np.float64)
        check(lib.polee_forest_get_nodes(self._h, ptr(off, i64p), ptr(feature, i32p), ptr(threshold, f64p), ptr(left, i32p),
                                         ptr(right, i32p), ptr(label, i32p)), self.ctx._h)
        return off, feature, threshold, left, right, label

    def set_nodes(self, nodes):
        """loads a forest built elsewhere (the host builder's, a hand-made one)"""
        off, feature, threshold, left, right, label = _node_arrays(nodes)
        if not (feature.size == threshold.size == left.size == right.size == label.size == (off[-1] if off.size else -1)):
            raise ValueError("node arrays of unequal length")
        if self.host:
            self._nodes = (off, feature, threshold, left, right, label)
            return
        check(_bind().polee_forest_set_nodes(self._h, off.size - 1, ptr(off, i64p), ptr(feature, i32p), ptr(threshold, f64p),
                                             ptr(left, i32p), ptr(right, i32p), ptr(label, i32p)), self.ctx._h)

    # ---- training
    def fit(self, x, labels, seed=DEFAULT_SEED):
        x = self._x(x)
        y = self._labels(labels, x.shape[0])
        if self.host:
            self._nodes = build_forest_host(x, y, self.k, seed, **self._opts_kw)
            return self
        check(_bind().polee_forest_fit_points(self._h, ptr(x, f32p), ptr(y, i32p), x.shape[0], C.c_uint64(seed & MASK)), self.ctx._h)
        return self

    def fit_sample(self, vars, labels, ndraws=20, draw_seed=DEFAULT_SEED, seed=DEFAULT_SEED + 1, z0=None):
        """trains on ndraws draws of every sample (row d S + s carries labels[s]); z0 f32 [ndraws, S, n-1] replaces the device's noise"""
        if self.host:
            raise ValueError("host=True takes points only: feed fit() the rows of log_draws()")
        ap = self._lik(vars)
        y = self._labels(labels, ap.S)
        z = z0_flat(z0, ndraws * ap.S * (ap.n - 1))
        check(_bind().polee_forest_fit(self._h, ap._h, ptr(y, i32p), int(ndraws), C.c_uint64(draw_seed & MASK), C.c_uint64(seed & MASK),
                                       ptr(z, f32p)), self.ctx._h)
        return self

    # ---- prediction
    def votes(self, x):
        """i32 [R, k]: trees per class"""
        x = self._x(x)
        if self.host:
            return forest_votes_host(self.nodes(), x, self.k)
        v = np.zeros((x.shape[0], self.k), np.int32)
        check(_bind().polee_forest_predict_points(self._h, ptr(x, f32p), x.shape[0], ptr(v, i32p)), self.ctx._h)
        return v

    def votes_sample(self, vars, ndraws=20, seed=DEFAULT_SEED + 2, z0=None):
        """i32 [S, k]: votes summed over ndraws draws of every sample"""
        if self.host:
            raise ValueError("host=True takes points only")
        ap = self._lik(vars)
        z = z0_flat(z0, ndraws * ap.S * (ap.n - 1))
        v = np.zeros((ap.S, self.k), np.int32)
        check(_bind().polee_forest_predict(self._h, ap._h, int(ndraws), C.c_uint64(seed & MASK), ptr(z, f32p), ptr(v, i32p)), self.ctx._h)
        return v

    def ntrees(self):
        return len(self.nodes()[0]) - 1

    def predict(self, x):
        """apply_forest_proba: votes / ntrees, f64 [R, k]"""
        return self.votes(x) / float(self.ntrees())

    def predict_sample(self, vars, ndraws=20, seed=DEFAULT_SEED + 2, z0=None):
        """votes / (ntrees ndraws), f64 [S, k] (random-forest.jl:263-270)"""
        return self.votes_sample(vars, ndraws, seed, z0) / float(self.ntrees() * int(ndraws))


# ---- kallisto bootstraps (models/kallisto.jl, random-forest.jl:207-234)
def read_kallisto_bootstrap_samples(filenames, pseudocount=0.0):
    """every bootstrap/bs* dataset of every file -> a list of log proportions [count_j, n]"""
    from . import h5io
    from .classify import counts_to_feature_log_props
    out = []
    for filename in filenames:
        with h5io.File(filename) as f:
            efflens = f.read("aux/eff_lengths", np.float64)
            rows, i = [], 0
            while f.exists("bootstrap/bs%d" % i):
                rows.append(counts_to_feature_log_props(f.read("bootstrap/bs%d" % i, np.float64).astype(np.float32), efflens, pseudocount))
                i += 1
        if not rows:
            raise ValueError("%s holds no bootstrap/bs* datasets" % filename)
        out.append(np.concatenate(rows, axis=0))
    return out


def bootstrap_training_set(boots, labels):
    """all bootstraps of all samples, each with its sample's label"""
    return np.concatenate(boots, axis=0), np.concatenate([np.full(b.shape[0], l, np.int32) for b, l in zip(boots, labels)])


def bootstrap_predict(forest, boots):
    """the mean over max-count passes of the forest's probabilities, sample j showing bootstrap i mod count_j in pass i"""
    passes = max(b.shape[0] for b in boots)
    y = np.zeros((len(boots), forest.k), np.float64)
    for i in range(passes):
        y += forest.predict(np.stack([b[i % b.shape[0]] for b in boots]))
    return y / passes


def parser():
    ap = argparse.ArgumentParser(prog="python -m polee_amd.random_forest", description=__doc__.split("\n\n")[0])
    ap.add_argument("training_experiment", metavar="training.yml", help="Training experiment specification")
    ap.add_argument("testing_experiment", metavar="testing.yml", help="Testing experiment specification")
    ap.add_argument("factor", help="Factor to classify by")
    ap.add_argument("--genes", action="store_true", help="(not built)")
    ap.add_argument("--ntrees", type=int, default=200, metavar="N", help="Number of trees")
    ap.add_argument("--nsubfeatures", type=float, default=10.0, metavar="C", help="Candidate features of a node: C sqrt(n)")
    ap.add_argument("--partial-sampling", type=float, default=1.0, metavar="P", help="Proportion of the rows in a tree's bootstrap")
    ap.add_argument("--training-samples", type=int, default=20, metavar="N", help="Draws per training sample")
    ap.add_argument("--testing-samples", type=int, default=20, metavar="N", help="Classify by the votes over N draws")
    ap.add_argument("--point-estimates", default=None, metavar="KEY",
                    help="Use point estimates (transcript_id,tpm CSVs) the experiments name under this key; needs --transcript-ids")
    ap.add_argument("--kallisto", action="store_true", help="Use kallisto maximum likelihood estimates (the samples' `kallisto` key)")
    ap.add_argument("--kallisto-bootstrap", action="store_true", help="Use kallisto bootstrap estimates")
    ap.add_argument("--pseudocount", type=float, default=None, metavar="C", help="With a point mode, add C tpm to each value")
    ap.add_argument("--seed", type=int, default=DEFAULT_SEED, metavar="N", help="RNG seed")
    ap.add_argument("--output-predictions", default="y-predicted.csv", metavar="filename", help="Output prediction probability matrix")
    ap.add_argument("--output-truth", default="y-true.csv", metavar="filename", help="Output true classes of the testing samples")
    ap.add_argument("--max-depth", type=int, default=-1, metavar="D", help="Deepest level of a tree (-1: no limit)")
    ap.add_argument("--min-samples-leaf", type=int, default=1, metavar="N", help="Fewest rows on either side of a split")
    ap.add_argument("--device", type=int, default=0, metavar="D", help="GPU to run on")
    ap.add_argument("--host", action="store_true", help="Build and predict on the host (point modes only; no GPU needed)")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (default 1..n)")
    return ap


def main(argv=None):
    a = parser().parse_args(sys.argv[1:] if argv is None else argv)
    if a.genes:
        raise SystemExit("--genes is not built (the reference sums logs of transcript draws there)")
    if a.kallisto and a.kallisto_bootstrap:
        raise SystemExit("Only one of '--kallisto' and '--kallisto-bootstrap' can be used.")
    if (a.kallisto or a.kallisto_bootstrap) and a.point_estimates is not None:
        raise SystemExit("'--point-estimates' is not compatible with '--kallisto' or '--kallisto-bootstrap'")
    point = a.kallisto or a.kallisto_bootstrap or a.point_estimates is not None
    if a.pseudocount is not None and not point:
        raise SystemExit("--pseudocount argument only valid with --point-estimates, --kallisto or --kallisto-bootstrap")
    if a.point_estimates is not None and not a.transcript_ids:
        raise SystemExit("--point-estimates needs --transcript-ids: the CSV rows are matched by transcript id")
    if a.host and not point:
        raise SystemExit("--host takes a point mode (--point-estimates, --kallisto, --kallisto-bootstrap): draws are made on the GPU")
    if a.ntrees < 1 or a.training_samples < 1 or a.testing_samples < 1:
        raise SystemExit("--ntrees, --training-samples and --testing-samples must be positive")
    from . import estimate, h5io
    from .classify import (build_factor_matrix, factor_names_of, load_point_estimates, log_point_estimates, read_kallisto_estimates,
                           write_classification_probs)
    from .pca import read_experiment
    from .sample import _read_lines
    training_spec, testing_spec = read_experiment(a.training_experiment), read_experiment(a.testing_experiment)
    for spec, name in ((training_spec, a.training_experiment), (testing_spec, a.testing_experiment)):
        if not spec.get("samples"):
            raise SystemExit("%s names no samples" % name)
    ctx = None
    if not a.host:
        from .core import Context
        ctx = Context(a.device)
    pc = 0.0 if a.pseudocount is None else a.pseudocount
    if a.kallisto or a.kallisto_bootstrap:
        _, _, f_train = estimate.read_specification(training_spec)
        _, _, f_test = estimate.read_specification(testing_spec)
        read = read_kallisto_bootstrap_samples if a.kallisto_bootstrap else read_kallisto_estimates
        x_train = read([s["kallisto"] for s in training_spec["samples"]], pc)
        x_test = read([s["kallisto"] for s in testing_spec["samples"]], pc)
        n = (x_train[0] if a.kallisto_bootstrap else x_train).shape[1]
    elif point:
        ids = _read_lines(a.transcript_ids)
        fn_train, _, f_train = estimate.read_specification(training_spec, point_estimates_key=a.point_estimates)
        fn_test, _, f_test = estimate.read_specification(testing_spec, point_estimates_key=a.point_estimates)
        x_train = log_point_estimates(load_point_estimates(fn_train, ids), a.pseudocount)
        x_test = log_point_estimates(load_point_estimates(fn_test, ids), a.pseudocount)
        n = x_train.shape[1]
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
    labels = y_train.argmax(axis=1).astype(np.int32)
    forest = RNASeqRandomForest(k, n, ctx=ctx, host=a.host, ntrees=a.ntrees, nsubfeatures=a.nsubfeatures,
                                partial_sampling=a.partial_sampling, max_depth=a.max_depth, min_samples_leaf=a.min_samples_leaf)
    try:
        if a.kallisto_bootstrap:
            xb, yb = bootstrap_training_set(x_train, labels)
            forest.fit(xb, yb, seed=a.seed + 1)
            y_predicted = bootstrap_predict(forest, x_test)
        elif point:
            forest.fit(x_train, labels, seed=a.seed + 1)
            y_predicted = forest.predict(x_test)
        else:
            forest.fit_sample(ls_train.variables, labels, a.training_samples, draw_seed=a.seed, seed=a.seed + 1)
            y_predicted = forest.predict_sample(ls_test.variables, a.testing_samples, seed=a.seed + 2)
    except L.NonFiniteError as e:
        raise SystemExit("%s\n(a point estimate of 0 has log -inf: give --pseudocount C)" % e)
    write_classification_probs(factor_names_of(factor_idx), a.output_predictions, a.output_truth, y_predicted, y_test)
    return 0


if __name__ == "__main__":
    sys.exit(main())

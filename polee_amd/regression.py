"""Host-side mirror of the regression model (models/polee_regression.py) over libpolee_hip's polee_regression_*.

Same class names, constructor arguments and return values as the reference; the TensorFlow-Probability
joint distributions and fit_surrogate_posterior are replaced by the device step in csrc/regression.hip.
Also: estimate_sample_scales (src/PoleeModel.jl:82-89) and the effect-size output semantics
(src/regression.jl:604-685).

`polee model regression` (src/regression.jl:19-601):

    python -m polee_amd.regression experiment.yml [--feature transcript | gene | gene-isoform] [--gene-pattern REGEX | --gene-annotations
        genes.yml] [--factors a,b] [--nonredundant] [--balanced] [--kallisto | --kallisto-bootstrap | --point-estimates KEY] ...

writes regression-coefficients.csv and, for gene-isoform, regression-isoform-coefficients.csv with the isoform effect sizes of
estimate_isoform_effect_sizes (:761-945), which run on the device (csrc/effects.hip).  Departures from the reference: factors and
options of the design matrix come in sorted order; genes come from --gene-pattern / --gene-annotations (no GFF reader); without
--isoform-effect-size, where the reference fails in log(abs(nothing)), prob_de is not computed and its column is left out;
--output-expression with --feature gene-isoform, where the reference fails on an undefined qx_loc, writes the genes' expression
(the gene block's qx_loc, labelled gene_id,gene_name); --feature splice-feature is not built.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import arr, check, f32p, ptr
from .core import RNASeqApproxLikelihood, default_context

# (name, shape code) of the flat parameter vector, in include/polee_hip.h's order
PARAM_TABLE = [
    ("qw_global_scale_variance_loc", "1"), ("qw_global_scale_variance_softplus_scale", "1"),
    ("qw_global_scale_noncentered_loc", "1"), ("qw_global_scale_noncentered_softplus_scale", "1"),
    ("qw_distortion_c_loc", "Fd"), ("qx_scale_concentration_c_loc", "d"), ("qx_scale_scale_c_loc", "d"),
    ("qw_local1_scale_variance_loc", "Fn"), ("qw_local1_scale_variance_softplus_scale", "Fn"),
    ("qw_local1_scale_noncentered_loc", "Fn"), ("qw_local1_scale_noncentered_softplus_scale", "Fn"),
    ("qw_local2_scale_variance_loc", "Fn"), ("qw_local2_scale_variance_softplus_scale", "Fn"),
    ("qw_local2_scale_noncentered_loc", "Fn"), ("qw_local2_scale_noncentered_softplus_scale", "Fn"),
    ("qw_loc", "Fn"), ("qw_softplus_scale", "Fn"),
    ("qx_bias_loc", "n"), ("qx_bias_softplus_scale", "n"),
    ("qx_scale_loc", "n"), ("qx_scale_softplus_scale", "n"),
    ("qx_loc", "Sn"), ("qx_softplus_scale", "Sn"),
]


def _softmax(a):
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def relaxed_onehot_terms(logits, y, T):
    """RelaxedOneHotCategorical(temperature T, logits) at y on the simplex (Maddison et al. 2017, eq. 10; TFP builds it as
    Exp(ExpRelaxedOneHotCategorical)):  log q(y) = lgamma(K) + (K - 1) log T + sum_k (logits_k - (T + 1) log y_k)
    - K logsumexp_k(logits_k - T log y_k).  Returns (log q [S], d log q / d logits at fixed y [S, K], d log q / d y [S, K])."""
    logits, y = np.asarray(logits, np.float64), np.asarray(y, np.float64)
    K = logits.shape[1]
    ly = np.log(y)
    u = logits - T * ly
    mx = u.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(u - mx).sum(axis=1))
    sm = np.exp(u - lse[:, None])
    lq = math.lgamma(K) + (K - 1) * math.log(T) + (logits - (T + 1.0) * ly).sum(axis=1) - K * lse
    return lq, 1.0 - K * sm, (-(T + 1.0) + K * T * sm) / y


def _softplus(x):
    return np.logaddexp(0.0, x).astype(np.float32)


def choose_knots(low, high, degree):
    """choose_knots (src/polee.py:69-76): `degree` hinges evenly inside (low, high)"""
    low, high, degree = float(low), float(high), int(degree)
    return np.array([low + (k + 1) * (high - low) / (degree + 1) for k in range(degree)], np.float32)


def estimate_sample_scales(x, upper_quantile=0.95):
    """src/PoleeModel.jl:82-89: per-sample offsets from the highly expressed features; x [S, n] log expression.
    Returns [S, 1] like the reference."""
    x = np.asarray(x, np.float64)
    x_mean = np.median(x, axis=0)
    high = x_mean > np.quantile(x_mean, upper_quantile)
    return np.median(x_mean[high][None, :] - x[:, high], axis=1, keepdims=True).astype(np.float32)


class RNASeqLinearRegression(L.Handle):
    """RNASeqLinearRegression (models/polee_regression.py:18-340).  `likelihood_model` is an
    RNASeqApproxLikelihood (or None with point estimates) instead of a TFP coroutine."""
    _destroy = "polee_regression_destroy"

    def __init__(self, F, x_init, likelihood_model, x_bias_loc0, x_bias_scale0, x_scale_hinges, sample_scales,
                 use_distortion, scale_penalty, use_point_estimates, kernel_regression_degree,
                 kernel_regression_bandwidth, ctx=None, comm=None, x_init_mean=None, normal_likelihood=None,
                 gene_likelihood=None):
        """comm / x_init_mean: samples sharded over ranks (polee_regression_set_comm) -- F, x_init, sample_scales are
        this rank's rows, x_init_mean the column means of x_init over all samples."""
        Fm = arr(np.atleast_2d(F), np.float32)
        x0 = arr(np.atleast_2d(x_init), np.float32)
        ss = arr(np.asarray(sample_scales).reshape(-1), np.float32)
        self.num_samples, self.num_factors = Fm.shape
        self.design = Fm
        self.num_features = x0.shape[1]
        if x0.shape[0] != self.num_samples or ss.size != self.num_samples:
            raise ValueError("F [S,F], x_init [S,n] and sample_scales [S] disagree on S")
        self.kernel_regression_degree = int(kernel_regression_degree)
        hg = None if x_scale_hinges is None else arr(np.asarray(x_scale_hinges).reshape(-1), np.float32)
        if hg is not None and hg.size != self.kernel_regression_degree:
            raise ValueError("x_scale_hinges must hold kernel_regression_degree values")
        self.use_point_estimates = bool(use_point_estimates)
        self.likelihood_model = likelihood_model
        # (kept for classify(): the testing model is created with the training model's settings)
        self._ctor = dict(x_bias_loc0=float(x_bias_loc0), x_bias_scale0=float(x_bias_scale0), use_distortion=bool(use_distortion),
                          scale_penalty=float(scale_penalty), kernel_regression_bandwidth=float(kernel_regression_bandwidth),
                          x_scale_hinges=None if hg is None else hg.copy(),
                          x_init_mean=(x0.astype(np.float64).mean(axis=0) if x_init_mean is None
                                       else np.asarray(x_init_mean, np.float64).reshape(-1)))
        if (not self.use_point_estimates and likelihood_model is None and normal_likelihood is None
                and gene_likelihood is None):
            raise ValueError("a likelihood model is needed unless use_point_estimates")
        if gene_likelihood is not None and ctx is None:
            ctx = gene_likelihood[0].ctx
        self.ctx = ctx or (likelihood_model.ctx if likelihood_model is not None else default_context())
        self._h = C.c_void_p()
        ap = likelihood_model._h if (likelihood_model is not None and not self.use_point_estimates) else None
        xm = None if x_init_mean is None else arr(np.asarray(x_init_mean).reshape(-1), np.float32)
        if xm is not None and xm.size != self.num_features:
            raise ValueError("x_init_mean must hold one value per feature")
        check(L.lib().polee_regression_create(
            self.ctx._h, ap, self.num_samples, self.num_factors, self.num_features, ptr(Fm, f32p), ptr(x0, f32p),
            ptr(xm, f32p), ptr(ss, f32p), ptr(hg, f32p), self.kernel_regression_degree, C.c_float(kernel_regression_bandwidth),
            C.c_float(x_bias_loc0), C.c_float(x_bias_scale0), int(bool(use_distortion)), C.c_float(scale_penalty),
            int(self.use_point_estimates), C.byref(self._h)), self.ctx._h)
        lib = L.lib()
        lib.polee_regression_num_params.restype = C.c_int64
        lib.polee_regression_num_noise.restype = C.c_int64
        lib.polee_regression_num_params.argtypes = [C.c_void_p]
        lib.polee_regression_num_noise.argtypes = [C.c_void_p]
        self.num_params = int(lib.polee_regression_num_params(self._h))
        self.num_noise = int(lib.polee_regression_num_noise(self._h))
        if normal_likelihood is not None:
            loc, scale = (arr(np.atleast_2d(a), np.float32) for a in normal_likelihood)
            if loc.shape != x0.shape or scale.shape != x0.shape:
                raise ValueError("the Normal likelihood's loc and scale must be [S, n]")
            check(lib.polee_regression_set_normal_likelihood(self._h, ptr(loc, f32p), ptr(scale, f32p)), self.ctx._h)
        self.num_isoform_params = 0
        if gene_likelihood is not None:  # (RNASeqApproxLikelihood over the transcripts, 0-based gene of each, init
            # [, isoform design: the gene-isoform model])
            lik, gene_of, xi0 = gene_likelihood[:3]
            Fi = arr(np.atleast_2d(gene_likelihood[3]), np.float32) if len(gene_likelihood) > 3 else None
            gene_of, xi0 = arr(gene_of, np.int32).reshape(-1), arr(np.atleast_2d(xi0), np.float32)
            if gene_of.size != lik.n or xi0.shape != (self.num_samples, lik.n):
                raise ValueError("gene_of must be [nt] and x_isoform_init [S, nt]")
            self.likelihood_model = lik
            if Fi is not None:
                if Fi.shape[0] != self.num_samples:
                    raise ValueError("F_isoform must be [S, Fi]")
                self.num_isoform_factors = Fi.shape[1]
                check(lib.polee_regression_set_gene_isoform_likelihood(
                    self._h, lik._h, ptr(gene_of, L.i32p), ptr(xi0, f32p), ptr(Fi, f32p), Fi.shape[1]), self.ctx._h)
            else:
                check(lib.polee_regression_set_gene_likelihood(self._h, lik._h, ptr(gene_of, L.i32p), ptr(xi0, f32p)),
                      self.ctx._h)
            lib.polee_regression_num_isoform_params.restype = C.c_int64
            lib.polee_regression_num_isoform_params.argtypes = [C.c_void_p]
            self.num_isoform_params = int(lib.polee_regression_num_isoform_params(self._h))
            self.num_noise = int(lib.polee_regression_num_noise(self._h))
        self.comm = comm
        if comm is not None:
            check(lib.polee_regression_set_comm(self._h, comm._h), self.ctx._h)

    # ---- parameters by the reference's variable names
    def _shape(self, code):
        S, F, n, d = self.num_samples, self.num_factors, self.num_features, self.kernel_regression_degree
        return {"1": (), "Fd": (F, d), "d": (d,), "Fn": (F, n), "n": (n,), "Sn": (S, n)}[code]

    def get_flat_params(self):
        p = np.empty(self.num_params, np.float32)
        check(L.lib().polee_regression_get_params(self._h, ptr(p, f32p)), self.ctx._h)
        return p

    def set_flat_params(self, p):
        p = arr(p, np.float32).reshape(-1)
        if p.size != self.num_params:
            raise ValueError("expected %d parameters" % self.num_params)
        check(L.lib().polee_regression_set_params(self._h, ptr(p, f32p)), self.ctx._h)

    def unflatten(self, vec):
        out, o = {}, 0
        for name, code in PARAM_TABLE:
            shp = self._shape(code)
            k = int(np.prod(shp)) if shp else 1
            out[name] = vec[o:o + k].reshape(shp)
            o += k
        return out

    def variables(self):
        """All surrogate-posterior variables (the reference's `<name>_var`) as a dict of arrays."""
        return self.unflatten(self.get_flat_params())

    def kernel_regression_weights(self):
        w = np.empty((self.kernel_regression_degree, self.num_features), np.float32)
        check(L.lib().polee_regression_weights(self._h, ptr(w, f32p)), self.ctx._h)
        return w

    def get_x_posterior_params(self):
        """models/polee_regression.py:121-122"""
        v = self.variables()
        return v["qx_loc"], _softplus(v["qx_softplus_scale"])

    def loss_and_gradients(self, noise=None, seed=123456789):
        """One evaluation of the variational loss and its gradient (flat), no update."""
        z = None if noise is None else arr(noise, np.float32).reshape(-1)
        if z is not None and z.size != self.num_noise:
            raise ValueError("expected %d noise values" % self.num_noise)
        loss = np.empty(1, np.float32)
        g = np.empty(self.num_params, np.float32)
        check(L.lib().polee_regression_eval(self._h, ptr(z, f32p), C.c_uint64(seed), ptr(loss, f32p), ptr(g, f32p)),
              self.ctx._h)
        return float(loss[0]), g

    # ---- isoform block of the gene-level model
    def get_isoform_params(self):
        p = np.empty(self.num_isoform_params, np.float32)
        check(L.lib().polee_regression_get_isoform_params(self._h, ptr(p, f32p)), self.ctx._h)
        return p

    def set_isoform_params(self, p):
        p = arr(p, np.float32).reshape(-1)
        if p.size != self.num_isoform_params:
            raise ValueError("expected %d isoform parameters" % self.num_isoform_params)
        check(L.lib().polee_regression_set_isoform_params(self._h, ptr(p, f32p)), self.ctx._h)

    def isoform_gradients(self):
        """Gradient of the isoform block left by the last loss_and_gradients()."""
        g = np.empty(self.num_isoform_params, np.float32)
        check(L.lib().polee_regression_get_isoform_grad(self._h, ptr(g, f32p)), self.ctx._h)
        return g

    # test hooks: the two halves of a step (include/polee_hip_debug.h)
    def _data_pass(self, noise):
        z = arr(noise, np.float32).reshape(-1)
        f = L.lib().polee_debug_regression_num_stats
        f.restype, f.argtypes = C.c_int64, [C.c_void_p]
        stats = np.empty(int(f(self._h)), np.float32)
        check(L.lib().polee_debug_regression_data_pass(self._h, ptr(z, f32p), ptr(stats, f32p)), self.ctx._h)
        return stats

    def _prior_pass(self, stats):
        st = arr(stats, np.float32).reshape(-1)
        loss, g = np.empty(1, np.float32), np.empty(self.num_params, np.float32)
        check(L.lib().polee_debug_regression_prior_pass(self._h, ptr(st, f32p), ptr(loss, f32p), ptr(g, f32p)),
              self.ctx._h)
        return float(loss[0]), g

    # ---- classify (models/polee_regression.py:342-413)
    def set_design(self, F):
        Fm = arr(np.atleast_2d(F), np.float32)
        if Fm.shape != (self.num_samples, self.num_factors):
            raise ValueError("the design matrix must be [S, F]")
        check(L.lib().polee_regression_set_design(self._h, ptr(Fm, f32p)), self.ctx._h)
        self.design = Fm

    def design_gradient(self):
        """d loss / d design [S, F] of the last evaluation or fit step (after set_design)."""
        g = np.empty((self.num_samples, self.num_factors), np.float32)
        check(L.lib().polee_regression_design_grad(self._h, ptr(g, f32p)), self.ctx._h)
        return g

    # ---- latent design (RNASeqPCA, models/polee_pca.py:14-92)
    def set_latent_design(self, z0, prior_scale=1.0):
        """The design matrix becomes a parameter z [S, F] with a Normal(0, prior_scale) prior and a point surrogate: every evaluation
        adds -log p(z), fit() trains z on the device, design_gradient() returns the total d loss / dz."""
        z = arr(np.atleast_2d(z0), np.float32)
        if z.shape != (self.num_samples, self.num_factors):
            raise ValueError("z0 must be [S, F]")
        check(L.lib().polee_regression_set_latent_design(self._h, ptr(z, f32p), C.c_float(prior_scale)), self.ctx._h)
        self.design = z

    def get_design(self):
        """The design matrix on the device, [S, F] (the trained z after set_latent_design)."""
        d = np.empty((self.num_samples, self.num_factors), np.float32)
        check(L.lib().polee_regression_get_design(self._h, ptr(d, f32p)), self.ctx._h)
        return d

    def _shared_size(self):
        """flat parameters in front of qx_loc: everything the samples share (the layout of include/polee_hip.h)"""
        F, n, d = self.num_factors, self.num_features, self.kernel_regression_degree
        return 4 + F * d + 2 * d + 10 * F * n + 4 * n

    def classify(self, x_init, likelihood_model, surrogate_likelihood_model, sample_scales, use_point_estimates, niter,
                 extra_training_vars=(), seed=123456789, return_trace=False):
        """classify (models/polee_regression.py:342-413): class probabilities [S_test, F] of testing samples under the FITTED model.
        Their design matrix is latent -- F ~ OneHotCategorical(uniform) per sample, surrogate RelaxedOneHotCategorical(T, logits)
        with the temperature annealed from 5 to 0.5 over the run (:385-391) -- everything the fitted model shares keeps its
        surrogate, and the trainable variables are the logits (+ the testing samples' qx_loc / qx_softplus_scale unless
        use_point_estimates), Adam at 1e-3 (:400).  `likelihood_model`: the testing samples' RNASeqApproxLikelihood (None with point
        estimates); `surrogate_likelihood_model` is part of the reference's signature only.  Per step the device model over the testing
        samples draws every latent but F, evaluates the loss and the gradients (polee_regression_fit, one step) and returns d loss / d F;
        the relaxed rows, their density and the logits' Adam are a few dozen numbers per step and stay on the host.
        Returns softmax(logits) (:407), with return_trace also the loss trace."""
        if extra_training_vars or isinstance(self, (RNASeqGeneLinearRegression, RNASeqGeneIsoformLinearRegression, RNASeqJointLinearRegression,
                                                    RNASeqNormalTranscriptLinearRegression)):
            raise NotImplementedError("classify is built for the transcript-level model (the one models/imputation.jl uses)")
        x0 = arr(np.atleast_2d(x_init), np.float32)
        S, K, n = x0.shape[0], self.num_factors, self.num_features
        c = self._ctor
        test = RNASeqLinearRegression(
            np.full((S, K), 1.0 / K, np.float32), x0, None if use_point_estimates else likelihood_model, c["x_bias_loc0"],
            c["x_bias_scale0"], c["x_scale_hinges"] if c["x_scale_hinges"] is not None else self._default_hinges(),
            sample_scales, c["use_distortion"], c["scale_penalty"], use_point_estimates, self.kernel_regression_degree,
            c["kernel_regression_bandwidth"], ctx=self.ctx, x_init_mean=c["x_init_mean"])
        ns = self._shared_size()
        flat = np.concatenate([self.get_flat_params()[:ns], x0.reshape(-1), np.full(S * n, -1.0, np.float32)]).astype(np.float32)
        test.set_flat_params(flat)
        lib = L.lib()
        check(lib.polee_regression_set_learning_rate(test._h, C.c_float(1e-3)), self.ctx._h)
        check(lib.polee_regression_set_trainable(test._h, C.c_int64(ns if not use_point_estimates else test.num_params),
                                                 C.c_int64(test.num_params)), self.ctx._h)
        rng = np.random.default_rng(seed)
        logits = np.zeros((S, K))
        m, v = np.zeros_like(logits), np.zeros_like(logits)
        trace = np.empty(int(niter), np.float64)
        for step in range(1, int(niter) + 1):
            T = 5.0 if step == 1 else 5.0 * 0.1 ** (step / float(niter))  # (trace_fn :385-391 anneals AFTER a step)
            gum = -np.log(-np.log(rng.uniform(1e-12, 1.0, size=(S, K))))
            y = _softmax((logits + gum) / T)
            test.set_design(y)
            dev_loss = test._fit_steps(1, seed + step)[0]
            lq, dl_direct, dl_dy = relaxed_onehot_terms(logits, y, T)
            dy = dl_dy + test.design_gradient().astype(np.float64)
            grad = dl_direct + (y * (dy - (y * dy).sum(axis=1, keepdims=True))) / T  # through y = softmax((logits + g) / T)
            trace[step - 1] = float(dev_loss) + lq.sum() + S * math.log(K)  # - log p(F) = log K per sample (uniform prior, :349-351)
            m = 0.9 * m + 0.1 * grad
            v = 0.999 * v + 0.001 * grad * grad
            lr_t = 1e-3 * math.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step)
            logits -= lr_t * m / (np.sqrt(v) + 1e-7)
        probs = _softmax(logits)
        return (probs, trace) if return_trace else probs

    def _fit_steps(self, niter, seed):
        """polee_regression_fit without the download of every variable that fit() returns: the loss trace only"""
        trace = np.empty(int(niter), np.float32)
        check(L.lib().polee_regression_fit(self._h, int(niter), C.c_uint64(seed), None, ptr(trace, f32p)), self.ctx._h)
        return trace

    def _default_hinges(self):
        """choose_knots (src/polee.py:69-76) over the training samples' column means, as polee_regression_create derives them"""
        mean = self._ctor["x_init_mean"]
        return choose_knots(mean.min(), mean.max(), self.kernel_regression_degree)

    def fit(self, niter, seed=123456789, noise=None, return_trace=False):
        """fit (models/polee_regression.py:303-340): returns (qx_loc, qw_loc, qw_scale, qx_bias_loc, qx_scale)."""
        z = None if noise is None else arr(noise, np.float32).reshape(-1)
        if z is not None and z.size != int(niter) * self.num_noise:
            raise ValueError("noise must hold niter x num_noise values")
        trace = np.empty(int(niter), np.float32)
        check(L.lib().polee_regression_fit(self._h, int(niter), C.c_uint64(seed), ptr(z, f32p), ptr(trace, f32p)),
              self.ctx._h)
        v = self.variables()
        out = (v["qx_loc"], v["qw_loc"], _softplus(v["qw_softplus_scale"]), v["qx_bias_loc"],
               _softplus(v["qx_scale_loc"]))
        return out + (trace,) if return_trace else out


class RNASeqTranscriptLinearRegression(RNASeqLinearRegression):
    """RNASeqTranscriptLinearRegression (models/polee_regression.py:422-460).  `vars`: the dict of
    create_tensorflow_variables! (estimate.jl:502-556) or an RNASeqApproxLikelihood."""

    def __init__(self, vars, x_init, F_arr, sample_scales, use_distortion, scale_penalty, use_point_estimates,
                 kernel_regression_degree=15, kernel_regression_bandwidth=1.0, ctx=None, comm=None, x_init_mean=None,
                 x_scale_hinges=None):
        x_init = np.asarray(x_init, np.float32)
        num_features = x_init.shape[1]
        lik = None
        if not use_point_estimates:
            lik = vars if isinstance(vars, RNASeqApproxLikelihood) else RNASeqApproxLikelihood(vars, ctx=ctx)
        super().__init__(F_arr, x_init, lik, math.log(1.0 / num_features), 12.0, x_scale_hinges, sample_scales,
                         use_distortion, scale_penalty, use_point_estimates, kernel_regression_degree,
                         kernel_regression_bandwidth, ctx=ctx, comm=comm, x_init_mean=x_init_mean)


    def classify(self, vars, x_init, sample_scales, use_point_estimates, niter, seed=123456789, return_trace=False):
        """classify (models/polee_regression.py:462-483, as models/imputation.jl:208-213 calls it): `vars` are the TESTING samples'
        likelihood variables (or their RNASeqApproxLikelihood); unused with point estimates."""
        lik = None
        if not use_point_estimates:
            lik = vars if isinstance(vars, RNASeqApproxLikelihood) else RNASeqApproxLikelihood(vars, ctx=self.ctx)
        return super().classify(x_init, lik, None, sample_scales, use_point_estimates, niter, seed=seed, return_trace=return_trace)


class RNASeqGeneLinearRegression(RNASeqLinearRegression):
    """RNASeqGeneLinearRegression (models/polee_regression.py:533-600): regression over gene expression with the
    transcript-level approximate likelihood reached through within-gene isoform log-expression.
    feature_idxs / transcript_idxs: the 1-based (gene, transcript) pairs of the reference; feature_sizes is unused
    (the reference only forwards it).  Built without point estimates only."""

    def __init__(self, vars, feature_idxs, transcript_idxs, x_gene_init, x_isoform_init, feature_sizes, F_arr,
                 sample_scales, use_distortion, scale_penalty, use_point_estimates, kernel_regression_degree=15,
                 kernel_regression_bandwidth=1.0, ctx=None):
        if use_point_estimates:
            raise NotImplementedError("the gene-level model is built without point estimates only")
        x_gene_init = np.asarray(x_gene_init, np.float32)
        lik = vars if isinstance(vars, RNASeqApproxLikelihood) else RNASeqApproxLikelihood(vars, ctx=ctx)
        fi = np.asarray(feature_idxs, np.int64).reshape(-1) - 1
        ti = np.asarray(transcript_idxs, np.int64).reshape(-1) - 1
        gene_of = np.full(lik.n, -1, np.int64)
        gene_of[ti] = fi
        if (gene_of < 0).any():
            raise ValueError("every transcript must belong to a gene")
        super().__init__(F_arr, x_gene_init, None, math.log(1.0 / x_gene_init.shape[1]), 12.0, None, sample_scales,
                         use_distortion, scale_penalty, False, kernel_regression_degree, kernel_regression_bandwidth,
                         ctx=ctx or lik.ctx, gene_likelihood=(lik, gene_of, x_isoform_init))

    def isoform_variables(self):
        v, S, nt = self.get_isoform_params(), self.num_samples, self.likelihood_model.n
        return dict(qx_isoform_mean_loc=v[:nt], qx_isoform_mean_softplus_scale=v[nt:2 * nt],
                    qx_isoform_loc=v[2 * nt:2 * nt + S * nt].reshape(S, nt),
                    qx_isoform_softplus_scale=v[2 * nt + S * nt:].reshape(S, nt))


class RNASeqGeneIsoformLinearRegression(RNASeqLinearRegression):
    """RNASeqGeneIsoformLinearRegression (models/polee_regression.py:656-877): regression over gene expression AND over
    the within-gene isoform mixtures (own design matrix F_isoform_arr, horseshoe+ coefficients).  Argument order and
    fit()'s return follow the reference.  Built without point estimates only."""

    # the isoform block in the order of the flat vector (include/polee_hip.h); shapes: 1, [Fi, nt], [nt], [S, nt]
    ISOFORM_PARAMS = [
        ("qw_isoform_global_scale_variance_loc", "1"), ("qw_isoform_global_scale_variance_softplus_scale", "1"),
        ("qw_isoform_global_scale_noncentered_loc", "1"), ("qw_isoform_global_scale_noncentered_softplus_scale", "1"),
        ("qw_isoform_local1_scale_variance_loc", "Ft"), ("qw_isoform_local1_scale_variance_softplus_scale", "Ft"),
        ("qw_isoform_local1_scale_noncentered_loc", "Ft"), ("qw_isoform_local1_scale_noncentered_softplus_scale", "Ft"),
        ("qw_isoform_local2_scale_variance_loc", "Ft"), ("qw_isoform_local2_scale_variance_softplus_scale", "Ft"),
        ("qw_isoform_local2_scale_noncentered_loc", "Ft"), ("qw_isoform_local2_scale_noncentered_softplus_scale", "Ft"),
        ("qw_isoform_loc", "Ft"), ("qw_isoform_softplus_scale", "Ft"),
        ("qx_isoform_bias_loc", "t"), ("qx_isoform_bias_softplus_scale", "t"),
        ("qx_isoform_scale_loc", "t"), ("qx_isoform_scale_softplus_scale", "t"),
        ("qx_isoform_loc", "St"), ("qx_isoform_softplus_scale", "St"),
    ]

    def __init__(self, vars, feature_idxs, transcript_idxs, x_gene_init, x_isoform_init, feature_sizes, F_gene_arr,
                 F_isoform_arr, sample_scales, use_distortion, scale_penalty, use_point_estimates,
                 kernel_regression_degree=15, kernel_regression_bandwidth=1.0, ctx=None):
        if use_point_estimates:
            raise NotImplementedError("the gene-isoform model is built without point estimates only")
        x_gene_init = np.asarray(x_gene_init, np.float32)
        lik = vars if isinstance(vars, RNASeqApproxLikelihood) else RNASeqApproxLikelihood(vars, ctx=ctx)
        fi = np.asarray(feature_idxs, np.int64).reshape(-1) - 1
        ti = np.asarray(transcript_idxs, np.int64).reshape(-1) - 1
        gene_of = np.full(lik.n, -1, np.int64)
        gene_of[ti] = fi
        if (gene_of < 0).any():
            raise ValueError("every transcript must belong to a gene")
        super().__init__(F_gene_arr, x_gene_init, None, math.log(1.0 / x_gene_init.shape[1]), 12.0, None, sample_scales,
                         use_distortion, scale_penalty, False, kernel_regression_degree, kernel_regression_bandwidth,
                         ctx=ctx or lik.ctx, gene_likelihood=(lik, gene_of, x_isoform_init, F_isoform_arr))

    def isoform_variables(self):
        v, S, nt, Fi = self.get_isoform_params(), self.num_samples, self.likelihood_model.n, self.num_isoform_factors
        shapes = {"1": (), "Ft": (Fi, nt), "t": (nt,), "St": (S, nt)}
        out, o = {}, 0
        for name, code in self.ISOFORM_PARAMS:
            k = int(np.prod(shapes[code], dtype=np.int64))
            out[name] = v[o:o + k].reshape(shapes[code])
            o += k
        assert o == v.size
        return out

    def fit(self, niter, seed=123456789, noise=None, return_trace=False):
        """fit (models/polee_regression.py:833-857): (qw_gene_loc, qw_gene_scale, qw_isoform_loc, qw_isoform_scale,
        qx_isoform_bias_loc, qx_isoform_bias_scale, qx_isoform_scale, qx_gene_bias_loc, qx_gene_scale,
        qx_gene_loc_factor_est)."""
        base = super().fit(niter, seed=seed, noise=noise, return_trace=True)
        _, qw_gene_loc, qw_gene_scale, qx_gene_bias_loc, qx_gene_scale, trace = base
        iv = self.isoform_variables()
        out = (qw_gene_loc, qw_gene_scale, iv["qw_isoform_loc"], _softplus(iv["qw_isoform_softplus_scale"]),
               iv["qx_isoform_bias_loc"], _softplus(iv["qx_isoform_bias_softplus_scale"]),
               _softplus(iv["qx_isoform_scale_loc"]), qx_gene_bias_loc, qx_gene_scale,
               self.design @ qw_gene_loc)
        return out + (trace,) if return_trace else out

    def write_other_params(self, output_filename):
        """write_other_params (models/polee_regression.py:859-875)"""
        iv = self.isoform_variables()
        with open(output_filename, "w") as output:
            for name in ("global_scale_variance_loc", "global_scale_variance_softplus_scale",
                         "global_scale_noncentered_loc", "global_scale_noncentered_softplus_scale"):
                output.write("qw_isoform_{}_var: {}\n".format(name, iv["qw_isoform_" + name]))


class RNASeqJointLinearRegression(RNASeqLinearRegression):
    """RNASeqJointLinearRegression (models/polee_regression.py:879-1283, driven by models/joint-regression.jl): regression
    over gene (TSS-group) expression AND over splice-feature usage, whose predictor reaches the transcripts through the 0/1
    feature matrix.  Argument order follows the reference: tss_is / tss_js = 1-based (transcript, gene) pairs,
    feature_is / feature_js = 1-based (transcript, splice feature) pairs.  fit() returns (qw_gene_loc, qw_gene_scale,
    qw_splice_loc, qw_splice_scale) (:1230-1234).  Built without point estimates only."""

    # the splice block of the isoform-parameter vector (include/polee_hip.h); shapes: 1, [F, P], [P]; then [nt], [S, nt]
    SPLICE_PARAMS = [
        ("qw_splice_global_scale_variance_loc", "1"), ("qw_splice_global_scale_variance_softplus_scale", "1"),
        ("qw_splice_global_scale_noncentered_loc", "1"), ("qw_splice_global_scale_noncentered_softplus_scale", "1"),
        ("qw_splice_local_scale_variance_loc", "FP"), ("qw_splice_local_scale_variance_softplus_scale", "FP"),
        ("qw_splice_local_scale_noncentered_loc", "FP"), ("qw_splice_local_scale_noncentered_softplus_scale", "FP"),
        ("_unused_local2_a", "FP"), ("_unused_local2_b", "FP"), ("_unused_local2_c", "FP"), ("_unused_local2_d", "FP"),
        ("qw_splice_loc", "FP"), ("qw_splice_softplus_scale", "FP"),
        ("qx_splice_bias_loc", "P"), ("qx_splice_bias_softplus_scale", "P"),
        ("_unused_scale_a", "P"), ("_unused_scale_b", "P"),
        ("qx_iso_scale_loc", "t"), ("qx_iso_scale_softplus_scale", "t"),
        ("qx_iso_loc", "St"), ("qx_iso_softplus_scale", "St"),
    ]

    def __init__(self, vars, tss_is, tss_js, num_gene_features, feature_is, feature_js, num_splice_features, gene_sizes,
                 x_gene_init, x_isoform_init, F_arr, sample_scales, use_point_estimates, kernel_regression_degree=15,
                 kernel_regression_bandwidth=1.0, ctx=None):
        if use_point_estimates:
            raise NotImplementedError("the joint model is built without point estimates only")
        x_gene_init = np.asarray(x_gene_init, np.float32)
        if x_gene_init.shape[1] != int(num_gene_features):
            raise ValueError("x_gene_init must be [S, num_gene_features]")
        lik = vars if isinstance(vars, RNASeqApproxLikelihood) else RNASeqApproxLikelihood(vars, ctx=ctx)
        ti = np.asarray(tss_is, np.int64).reshape(-1) - 1
        gi = np.asarray(tss_js, np.int64).reshape(-1) - 1
        gene_of = np.full(lik.n, -1, np.int64)
        gene_of[ti] = gi
        if (gene_of < 0).any():
            raise ValueError("every transcript must belong to a gene feature")
        # the gene block: no distortion (:1029), scale-drift penalty Normal(0, 5e-4) (:1052-1054)
        super().__init__(F_arr, x_gene_init, None, math.log(1.0 / int(num_gene_features)), 12.0, None, sample_scales, False,
                         5e-4, False, kernel_regression_degree, kernel_regression_bandwidth, ctx=ctx or lik.ctx,
                         gene_likelihood=(lik, gene_of, x_isoform_init))
        # (the base constructor attaches the plain gene-level likelihood; polee_regression_set_joint_likelihood below
        # re-attaches it and replaces its isoform block by the joint model's splice block)
        xi0 = arr(np.atleast_2d(x_isoform_init), np.float32)
        if xi0.shape != (self.num_samples, lik.n):
            raise ValueError("x_isoform_init must be [S, nt]")
        pt = arr(np.asarray(feature_is, np.int64).reshape(-1) - 1, np.int32)
        pf = arr(np.asarray(feature_js, np.int64).reshape(-1) - 1, np.int32)
        if pt.size != pf.size:
            raise ValueError("feature_is and feature_js must pair up")
        self.num_splice_features = int(num_splice_features)
        self.likelihood_model = lik
        lib = L.lib()
        check(lib.polee_regression_set_joint_likelihood(self._h, lik._h, ptr(arr(gene_of, np.int32), L.i32p), ptr(xi0, f32p),
                                                        self.num_splice_features, ptr(pt, L.i32p), ptr(pf, L.i32p),
                                                        C.c_int64(pt.size)), self.ctx._h)
        lib.polee_regression_num_isoform_params.restype = C.c_int64
        lib.polee_regression_num_isoform_params.argtypes = [C.c_void_p]
        self.num_isoform_params = int(lib.polee_regression_num_isoform_params(self._h))
        self.num_noise = int(lib.polee_regression_num_noise(self._h))

    def splice_variables(self):
        v, S, nt, F, P = (self.get_isoform_params(), self.num_samples, self.likelihood_model.n, self.num_factors,
                          self.num_splice_features)
        shapes = {"1": (), "FP": (F, P), "P": (P,), "t": (nt,), "St": (S, nt)}
        out, o = {}, 0
        for name, code in self.SPLICE_PARAMS:
            k = int(np.prod(shapes[code], dtype=np.int64))
            out[name] = v[o:o + k].reshape(shapes[code])
            o += k
        assert o == v.size
        return out

    def fit(self, niter, seed=123456789, noise=None, return_trace=False):
        """fit (models/polee_regression.py:1204-1234): (qw_gene_loc, qw_gene_scale, qw_splice_loc, qw_splice_scale)."""
        base = super().fit(niter, seed=seed, noise=noise, return_trace=True)
        _, qw_gene_loc, qw_gene_scale, _, _, trace = base
        sv = self.splice_variables()
        out = (qw_gene_loc, qw_gene_scale, sv["qw_splice_loc"], _softplus(sv["qw_splice_softplus_scale"]))
        return out + (trace,) if return_trace else out


class RNASeqNormalTranscriptLinearRegression(RNASeqLinearRegression):
    """RNASeqNormalTranscriptLinearRegression (models/polee_regression.py:490-531): point estimates and their standard
    deviation in place of the approximate likelihood.  `vars` is unused, as in the reference."""

    def __init__(self, vars, x_likelihood_loc, x_likelihood_scale, F_arr, sample_scales, use_distortion, scale_penalty,
                 kernel_regression_degree=15, kernel_regression_bandwidth=1.0, ctx=None, comm=None, x_init_mean=None):
        loc = np.asarray(x_likelihood_loc, np.float32)
        super().__init__(F_arr, loc, None, math.log(1.0 / loc.shape[1]), 12.0, None, sample_scales, use_distortion,
                         scale_penalty, False, kernel_regression_degree, kernel_regression_bandwidth, ctx=ctx, comm=comm,
                         x_init_mean=x_init_mean, normal_likelihood=(loc, x_likelihood_scale))


# ---- output semantics (src/regression.jl:604-685)
def find_minimum_effect_size(mu, sigma, target_coverage):
    """Bisection of src/regression.jl:604-622 on P(|w| < delta) under Normal(mu, sigma)."""
    from scipy.stats import norm
    lo, hi, coverage = 0.0, 20.0, 1.0
    while abs(coverage - target_coverage) / target_coverage > 0.001:
        d = (hi + lo) / 2
        coverage = norm.cdf(d, mu, sigma) - norm.cdf(-d, mu, sigma)
        if coverage > target_coverage:
            hi = d
        else:
            lo = d
        if hi - lo < 1e-15:
            break
    return (hi + lo) / 2


def write_regression_effects(output_filename, factor_names, feature_names_label, feature_names, qx_bias, qx_scale,
                             qw_loc, qw_scale, q0, q1, effect_size, mes_target_coverage,
                             write_variational_posterior_params=False):
    """write_regression_effects (src/regression.jl:625-685): CSV of effect sizes in log2 units with t_10 credible
    intervals and the minimum effect size."""
    from scipy.stats import t as tdist
    qw_loc, qw_scale = np.asarray(qw_loc), np.asarray(qw_scale)
    assert qw_loc.shape == qw_scale.shape
    num_factors, num_features = qw_loc.shape
    ln2 = math.log(2.0)
    tq0, tq1 = tdist.ppf(q0, 10.0), tdist.ppf(q1, 10.0)
    es = None if effect_size is None else math.log(abs(effect_size))
    with open(output_filename, "w") as out:
        out.write("factor,%s,min_effect_size,mean_effect_size,lower_credible,upper_credible" % feature_names_label)
        if es is not None:
            out.write(",prob_de,prob_down_de,prob_up_de")
        if write_variational_posterior_params:
            out.write(",qx_bias_loc,qx_scale,qw_loc,qw_scale")
        out.write("\n")
        for i in range(num_factors):
            for j in range(num_features):
                loc, sc = float(qw_loc[i, j]), float(qw_scale[i, j])
                mes = find_minimum_effect_size(loc, sc, mes_target_coverage)
                out.write("%s,%s,%f,%f,%f,%f" % (factor_names[i], feature_names[j], mes / ln2, loc / ln2,
                                                 (tq0 * sc + loc) / ln2, (tq1 * sc + loc) / ln2))
                if es is not None:
                    down = tdist.cdf((-es - loc) / sc, 10.0)
                    up = tdist.sf((es - loc) / sc, 10.0)
                    out.write(",%f,%f,%f" % (max(down, up), down, up))
                if write_variational_posterior_params:
                    out.write(",%f,%f,%f,%f" % (qx_bias[j], qx_scale[j], loc, sc))
                out.write("\n")


# ---- isoform effect sizes (src/regression.jl:761-945; csrc/effects.hip)
EFFECT_DRAWS = 1000      # niter of estimate_isoform_effect_sizes (:766)
MAX_EFFECT_DRAWS = 4096  # the kernel keeps 28 bytes of LDS per draw (csrc/effects.hip)
DEFAULT_SEED = 123456789
_MASK = (1 << 64) - 1


class IsoformEffects(L.Handle):
    """The device handle polee_effects_* (include/polee_hip.h): the transcripts of n are segmented by gene once; run() makes the
    Monte-Carlo draws and returns the six arrays.  gene_of: the 0-based gene of every transcript, in any order."""
    _destroy = "polee_effects_destroy"

    def __init__(self, gene_of, num_genes, num_factors, ctx=None):
        g = arr(np.asarray(gene_of).reshape(-1), np.int32)
        self.n, self.G, self.F = g.size, int(num_genes), int(num_factors)
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        self.kernel_ms = None
        check(L.lib().polee_effects_create(self.ctx._h, self.n, self.G, ptr(g, L.i32p), self.F, C.byref(self._h)), self.ctx._h)

    def run(self, qw_loc, qw_scale, qx_bias_loc, qx_bias_scale, niter=EFFECT_DRAWS, target_coverage=0.1, effect_size=None,
            aitchison_effect_size=None, seed=DEFAULT_SEED, zx=None, zw=None):
        """(min_effect_sizes, mean_effect_sizes, prob_de [F, n], aitchison_min, aitchison_mean, aitchison_prob_de [F, G]), f32; a
        prob_de whose threshold is None is None.  effect_size is compared as given (the caller takes log |S|).  zx [niter, n] and
        zw [niter, F, n] replace the device's noise.  self.kernel_ms: the kernel's time between two stream events."""
        F, n, G = self.F, self.n, self.G
        wl, ws = arr(np.atleast_2d(qw_loc), np.float32), arr(np.atleast_2d(qw_scale), np.float32)
        bl, bs = arr(qx_bias_loc, np.float32).reshape(-1), arr(qx_bias_scale, np.float32).reshape(-1)
        if wl.shape != (F, n) or ws.shape != (F, n) or bl.size != n or bs.size != n:
            raise ValueError("expected qw_loc and qw_scale [%d, %d], qx_bias_loc and qx_bias_scale [%d]" % (F, n, n))
        zx = None if zx is None else arr(zx, np.float32).reshape(-1)
        zw = None if zw is None else arr(zw, np.float32).reshape(-1)
        out = [np.empty((F, n), np.float32) for _ in range(3)] + [np.empty((F, G), np.float32) for _ in range(3)]
        nan = float("nan")
        ms = C.c_double(0.0)
        check(L.lib().polee_effects_run(
            self._h, ptr(wl, f32p), ptr(ws, f32p), ptr(bl, f32p), ptr(bs, f32p), C.c_int32(int(niter)), C.c_double(target_coverage),
            C.c_double(nan if effect_size is None else effect_size),
            C.c_double(nan if aitchison_effect_size is None else aitchison_effect_size), C.c_uint64(int(seed) & _MASK),
            ptr(zx, f32p), C.c_int64(0 if zx is None else zx.size), ptr(zw, f32p), C.c_int64(0 if zw is None else zw.size),
            *[ptr(o, f32p) for o in out], C.byref(ms)), self.ctx._h)
        self.kernel_ms = ms.value
        if effect_size is None:
            out[2] = None
        if aitchison_effect_size is None:
            out[5] = None
        return tuple(out)


def _gene_of(gene_idxs, transcript_idxs, n):
    """the 0-based gene of every transcript from the reference's 1-based (gene, transcript) pairs"""
    gi = np.asarray(gene_idxs, np.int64).reshape(-1) - 1
    ti = np.asarray(transcript_idxs, np.int64).reshape(-1) - 1
    gene_of = np.full(n, -1, np.int64)
    gene_of[ti] = gi
    if (gene_of < 0).any():
        raise ValueError("every transcript must belong to a gene")
    return gene_of


def estimate_isoform_effect_sizes(gene_idxs, transcript_idxs, effect_size, aitchison_effect_size, qw_loc, qw_scale, qx_bias_loc,
                                  qx_bias_scale, qx_gene_loc_factor_est=None, niter=EFFECT_DRAWS, target_coverage=0.1,
                                  seed=DEFAULT_SEED, zx=None, zw=None, ctx=None):
    """estimate_isoform_effect_sizes (src/regression.jl:761-945) on the device, the reference's argument order and six return values:
    (min_effect_sizes, mean_effect_sizes, prob_de, aitchison_min_effect_sizes, aitchison_mean_effect_sizes, aitchison_prob_de).
    gene_idxs / transcript_idxs are the 1-based pairs of gene_map.  effect_size is on the log scale already (main passes
    log |--isoform-effect-size|); with None -- where the reference fails in log(abs(nothing)) -- prob_de is None.  prob_de is
    one-sided, #{e > effect_size} / niter, as the reference computes it (:850).  qx_gene_loc_factor_est is accepted and IGNORED: the
    reference only feeds two values from it that nothing reads (expr, expr_alt, :843-844).  The evaluation is in log space, so a gene
    whose bias spans more than ~700 stays finite where the reference's exp / normalise / log gives log 0."""
    qw_loc = np.atleast_2d(np.asarray(qw_loc, np.float32))
    F, n = qw_loc.shape
    num_genes = int(np.max(gene_idxs))
    fx = IsoformEffects(_gene_of(gene_idxs, transcript_idxs, n), num_genes, F, ctx=ctx)
    return fx.run(qw_loc, qw_scale, qx_bias_loc, qx_bias_scale, niter=niter, target_coverage=target_coverage, effect_size=effect_size,
                  aitchison_effect_size=aitchison_effect_size, seed=seed, zx=zx, zw=zw)


# ---- the design matrix (src/PoleeModel.jl:165-232)
def build_design_matrix(sample_factors, factors=None, nonredundant=None, balanced=False):
    """build_factor_matrix (src/PoleeModel.jl:165-232) for several factors: (F f32 [S, columns], factor_names), names `factor:option`.
    The reference iterates a Dict of Sets, whose order is arbitrary; here factors and options come in SORTED order (the decision of
    classify.build_factor_matrix).  A sample without a factor has the option "missing".  nonredundant: None keeps every option; ""
    drops "missing" where it is an option, else the first sorted option; a name drops that option where it occurs.  balanced:
    0 becomes -1 (src/regression.jl:254-260)."""
    sample_factors = [{str(k): str(v) for k, v in (f or {}).items()} for f in sample_factors]
    if factors is None:
        factors = sorted({k for f in sample_factors for k in f})
    else:
        factors = sorted(set(str(f) for f in factors))
    columns = []
    for factor in factors:
        options = sorted({f.get(factor, "missing") for f in sample_factors})
        if nonredundant is not None:
            if nonredundant != "":
                options = [o for o in options if o != nonredundant]
            elif "missing" in options:
                options.remove("missing")
            elif options:
                options = options[1:]
        columns += [(factor, o) for o in options]
    F = np.zeros((len(sample_factors), len(columns)), np.float32)
    for c, (factor, option) in enumerate(columns):
        for i, f in enumerate(sample_factors):
            if f.get(factor, "missing") == option:
                F[i, c] = 1.0
    if balanced:
        F[F == 0] = -1.0
    return F, ["%s:%s" % c for c in columns]


# ---- genes without a GFF reader (src/rnaseq_sample.jl:229-250, src/transcripts.jl:956-1040)
def gene_map(transcript_ids, pattern=None, annotations=None):
    """populate_ts_metadata! + gene_feature_matrix: (num_genes, gene_idxs, transcript_idxs, gene_ids, gene_names), the two index lists
    1-based and sorted by transcript, as the model classes expect.  pattern: a regular expression searched in every transcript id; the
    gene id is its first capture group, or the whole match without one; a transcript it does not match becomes a gene of its own,
    `unknown-gene-K`, K counting such transcripts from 1 (:244-247).  annotations: the parsed --gene-annotations file, a list of
    {gene_name, transcripts}; a transcript no entry names is an error (the reference fails on the missing key).  Genes are numbered in
    order of first appearance (the reference: the order of a Dict).  gene_names are empty, as in the reference without a GFF."""
    import re
    ids = [str(t) for t in transcript_ids]
    if (pattern is None) == (annotations is None):
        raise ValueError("exactly one of pattern and annotations is needed")
    if annotations is not None:
        by_transcript = {}
        for entry in annotations:
            for t in entry["transcripts"]:
                by_transcript[str(t)] = str(entry["gene_name"])
        missing = [t for t in ids if t not in by_transcript]
        if missing:
            raise ValueError("the gene annotations name no gene for %d transcripts (first: %s)" % (len(missing), missing[0]))
        gids = [by_transcript[t] for t in ids]
    else:
        rx, unknown, gids = re.compile(pattern), 0, []
        for t in ids:
            mat = rx.search(t)
            if mat is not None:
                gids.append(mat.group(1) if rx.groups else mat.group(0))
            else:
                unknown += 1
                gids.append("unknown-gene-%d" % unknown)
    nums = {}
    for gid in gids:
        nums.setdefault(gid, len(nums) + 1)
    gene_idxs = np.array([nums[gid] for gid in gids], np.int64)
    transcript_idxs = np.arange(1, len(ids) + 1, dtype=np.int64)
    gene_ids = list(nums)
    return len(nums), gene_idxs, transcript_idxs, gene_ids, [""] * len(nums)


def gene_initial_values(gene_idxs, transcript_idxs, x_init, num_samples, num_features, n):
    """gene_initial_values (src/PoleeModel.jl:240-263): (x_gene_init [S, G], x_isoform_init [S, n]) in Float32 -- the log of the genes'
    summed expression and of the isoforms' shares of it"""
    x_init = np.asarray(x_init, np.float32)
    gi = np.asarray(gene_idxs, np.int64).reshape(-1) - 1
    ti = np.asarray(transcript_idxs, np.int64).reshape(-1) - 1
    x_gene = np.zeros((int(num_samples), int(num_features)), np.float32)
    x_iso = np.zeros((int(num_samples), int(n)), np.float32)
    for i in range(int(num_samples)):
        np.add.at(x_gene[i], gi, x_init[i, ti])  # (Float32 sums in the pairs' order, as the reference's loop)
        x_iso[i, ti] = x_init[i, ti] / x_gene[i, gi]
    with np.errstate(divide="ignore"):
        return np.log(x_gene), np.log(x_iso)


# ---- writers (src/regression.jl:380-419, 573-587, 688-758); print(::Float32) through pca._julia_float
def write_isoform_regression_effects(output_filename, gene_idxs, transcript_idxs, factor_names, gene_ids, gene_names, transcript_names,
                                     min_effect_sizes, mean_effect_sizes, prob_de, qw_isoform_loc, qx_isoform_bias_loc, qx_isoform_scale):
    """write_isoform_regression_effects (src/regression.jl:688-729); the prob_de column is left out when prob_de is None"""
    from .pca import _julia_float as jf
    min_effect_sizes = np.asarray(min_effect_sizes)
    num_factors, n = min_effect_sizes.shape
    gene_of = _gene_of(gene_idxs, transcript_idxs, n)
    with open(output_filename, "w") as out:
        out.write("factor,gene_id,gene_name,transcript_id,mean_effect_size,min_effect_size")
        if prob_de is not None:
            out.write(",prob_de")
        out.write(",w_mean,x_bias,x_scale\n")
        for i in range(num_factors):
            for j in range(n):
                g = gene_of[j]
                row = [str(factor_names[i]), str(gene_ids[g]), str(gene_names[g]), str(transcript_names[j]),
                       jf(mean_effect_sizes[i][j]), jf(min_effect_sizes[i][j])]
                if prob_de is not None:
                    row.append(jf(prob_de[i][j]))
                row += [jf(qw_isoform_loc[i][j]), jf(qx_isoform_bias_loc[j]), jf(qx_isoform_scale[j])]
                out.write(",".join(row) + "\n")


def write_aitchison_results(output_filename, factor_names, gene_ids, gene_names, min_effect_sizes, mean_effect_sizes, prob_de):
    """write_aitchison_results (src/regression.jl:732-758)"""
    from .pca import _julia_float as jf
    min_effect_sizes = np.asarray(min_effect_sizes)
    num_factors, num_genes = min_effect_sizes.shape
    with open(output_filename, "w") as out:
        out.write("factor,gene_id,gene_name,mean_effect_size,min_effect_size")
        if prob_de is not None:
            out.write(",prob_de")
        out.write("\n")
        for i in range(num_factors):
            for j in range(num_genes):
                row = [str(factor_names[i]), str(gene_ids[j]), str(gene_names[j]), jf(mean_effect_sizes[i][j]), jf(min_effect_sizes[i][j])]
                if prob_de is not None:
                    row.append(jf(prob_de[i][j]))
                out.write(",".join(row) + "\n")


def write_expression(output_filename, feature_names_label, feature_names, sample_names, qx_loc):
    """--output-expression (src/regression.jl:573-587): TPM = 1e6 softmax(qx_loc) per sample, feature-major rows"""
    from .pca import _julia_float as jf
    x = np.exp(np.asarray(qx_loc, np.float32))
    x = x / x.sum(axis=1, keepdims=True, dtype=np.float32)
    x = (x * np.float32(1e6)).astype(np.float32)
    with open(output_filename, "w") as out:
        out.write("%s,sample,tpm\n" % feature_names_label)
        for j in range(x.shape[1]):
            for i in range(x.shape[0]):
                out.write("%s,%s,%s\n" % (feature_names[j], sample_names[i], jf(x[i, j])))


def write_x_init(output_filename, label, names, x_init_log):
    """--x-isoform-init-output / --x-gene-init-output (src/regression.jl:380-419): exp of the initial values, one row per feature"""
    from .pca import _julia_float as jf
    x = np.exp(np.asarray(x_init_log, np.float32))
    with open(output_filename, "w") as out:
        out.write(label + "".join(",x%d" % (i + 1) for i in range(x.shape[0])) + "\n")
        for j, name in enumerate(names):
            out.write(str(name) + "".join("," + jf(v) for v in x[:, j]) + "\n")


# ---- kallisto estimates (src/estimate.jl:66-146)
def _kallisto_proportions(counts, efflens, pseudocount, file_ids, transcript_idx, n):
    """kallisto_counts_to_proportions (src/estimate.jl:66-79): Float32 counts / effective lengths placed by transcript id, normalised,
    + pseudocount / 1e6; [n]"""
    xs = np.zeros(n, np.float32)
    vals = (np.asarray(counts, np.float32) / np.asarray(efflens, np.float64)).astype(np.float32)
    if file_ids is None:
        xs[:] = vals
    else:
        for t, v in zip(file_ids, vals):
            j = transcript_idx.get(t)
            if j is not None:
                xs[j] = v
    xs = xs / xs.sum(dtype=np.float32)
    return (xs + np.float32(pseudocount / np.float32(1e6))).astype(np.float32)


def load_kallisto_estimates(filenames, pseudocount=0.0, use_bootstrap=False, transcript_ids=None):
    """load_kallisto_estimates_from_specification (src/estimate.jl:86-146) over kallisto's abundance.h5 files: (x0 f32 [S, n],
    log_x0_std f32 [S, n] or None).  With use_bootstrap, per transcript the mean and the standard deviation (n - 1 in the denominator,
    Julia's std) of the log bootstrap proportions, the latter floored at 0.5, and x0 = exp(mean); these feed
    RNASeqNormalTranscriptLinearRegression.  The bootstrap datasets are bootstrap/bs0, bs1, ... as kallisto names them.
    transcript_ids: place the files' rows by aux/ids (transcripts a file does not name stay 0); None takes the files' own order."""
    from . import h5io
    idx = None if transcript_ids is None else {str(t): j for j, t in enumerate(transcript_ids)}
    xss, stds = [], []
    for filename in filenames:
        with h5io.File(filename) as f:
            efflens = f.read("aux/eff_lengths", np.float64)
            file_ids = f.read_strings("aux/ids") if idx is not None else None
            n = efflens.size if idx is None else len(idx)
            if not use_bootstrap:
                xss.append(_kallisto_proportions(f.read("est_counts", np.float64), efflens, pseudocount, file_ids, idx, n))
                continue
            bss, b = [], 0
            while f.exists("bootstrap/bs%d" % b):
                bss.append(_kallisto_proportions(f.read("bootstrap/bs%d" % b, np.float64), efflens, pseudocount, file_ids, idx, n))
                b += 1
            if len(bss) < 2:
                raise ValueError("%s holds %d bootstrap samples; a standard deviation needs two" % (filename, len(bss)))
            with np.errstate(divide="ignore", invalid="ignore"):
                log_bs = np.log(np.stack(bss)).astype(np.float32)
                stds.append(np.maximum(np.float32(0.5), log_bs.std(axis=0, ddof=1, dtype=np.float64).astype(np.float32)))
                xss.append(np.exp(log_bs.mean(axis=0, dtype=np.float64).astype(np.float32)))
    return np.stack(xss).astype(np.float32), (np.stack(stds).astype(np.float32) if use_bootstrap else None)


# ---- the command line (src/regression.jl:19-601)
NUM_STEPS = {"transcript": 6000, "gene": 10000, "gene-isoform": 6000}  # (:327, :295, :433)


def parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m polee_amd.regression",
                                 description="`polee model regression` on the GPU: a linear regression over transcript, gene or "
                                             "gene and isoform expression (src/regression.jl)")
    ap.add_argument("experiment", metavar="experiment.yml", help="Experiment specification")
    ap.add_argument("--feature", default="transcript", metavar="F", help="One of transcript, gene, gene-isoform (splice-feature is not built)")
    ap.add_argument("--point-estimates", default=None, metavar="KEY",
                    help="Use point estimates (transcript_id,tpm CSVs) the experiment names under this key; needs --transcript-ids")
    ap.add_argument("--kallisto-bootstrap", action="store_true", help="Use kallisto bootstrap samples (the samples' `kallisto` key)")
    ap.add_argument("--kallisto", action="store_true", help="Use kallisto maximum likelihood estimates (the samples' `kallisto` key)")
    ap.add_argument("--gene-pattern", default=None, metavar="regex", help="A regular expression extracting gene ids from transcript ids")
    ap.add_argument("--gene-annotations", default=None, metavar="filename", help="YAML file assigning transcript ids to genes")
    ap.add_argument("--pseudocount", type=float, default=None, metavar="C", help="With point estimates, add C tpm to each value")
    ap.add_argument("--output", default="regression-coefficients.csv", metavar="filename", help="Output file for regression coefficients")
    ap.add_argument("--isoform-output", default="regression-isoform-coefficients.csv", metavar="filename",
                    help="Output file for isoform regression results of gene-isoform regression")
    ap.add_argument("--aitchison-distance-output", default=None, metavar="filename",
                    help="Output the Aitchison distances, a test for overall isoform composition changes")
    ap.add_argument("--aitchison-distance-effect-size", type=float, default=1.0, metavar="S")
    ap.add_argument("--extra-params-output", default=None, metavar="filename", help="Output some additional parameter values")
    ap.add_argument("--output-expression", default=None, metavar="filename", help="Output expression estimates to the given file")
    ap.add_argument("--lower-credible", type=float, default=0.025, metavar="L")
    ap.add_argument("--upper-credible", type=float, default=0.975, metavar="U")
    ap.add_argument("--min-effect-size-coverage", type=float, default=0.1, metavar="C")
    ap.add_argument("--write-variational-posterior-params", action="store_true")
    ap.add_argument("--effect-size", type=float, default=None, metavar="S",
                    help="Output the posterior probability of abs fold-change greater than S")
    ap.add_argument("--isoform-effect-size", type=float, default=None, metavar="S",
                    help="Output the posterior probability of an isoform log-ratio greater than log S")
    ap.add_argument("--x-isoform-init-output", default=None, metavar="filename")
    ap.add_argument("--x-gene-init-output", default=None, metavar="filename")
    ap.add_argument("--factors", default=None, help="Comma-separated list of factors to regress on (default: all)")
    ap.add_argument("--no-distortion", action="store_true", help="Disable the 'distortion' model")
    ap.add_argument("--scale-penalty", type=float, default=1e-3, help="Std. dev. of the penalty on expression vectors straying from sum 1")
    ap.add_argument("--nonredundant", action="store_true", help="Exclude one option of each factor")
    ap.add_argument("--redundant-factor", default="", metavar="factor", help="With --nonredundant, exclude this option")
    ap.add_argument("--balanced", action="store_true", help="-1/1 instead of 0/1 in the design matrix")
    ap.add_argument("--transformation", default=None, metavar="polee-transform.h5", help="A Polya tree shared by the samples")
    ap.add_argument("--num-steps", type=int, default=None, metavar="N", help="Optimiser steps (default 6000; 10000 for --feature gene)")
    ap.add_argument("--effect-draws", type=int, default=EFFECT_DRAWS, metavar="N", help="Monte-Carlo draws of the isoform effect sizes")
    ap.add_argument("--seed", type=int, default=DEFAULT_SEED, metavar="N", help="RNG seed")
    ap.add_argument("--device", type=int, default=0, metavar="D", help="GPU to run on")
    ap.add_argument("--transcript-ids", metavar="ids.txt", help="Transcript ids, one per line (default 1..n)")
    return ap


def main(argv=None):
    import sys
    a = parser().parse_args(sys.argv[1:] if argv is None else argv)
    feature = a.feature
    if feature == "splice-feature":
        raise SystemExit("--feature splice-feature is not built: it needs the reference's GFF-derived splicing features "
                         "(DESIGN.md section 7)")
    if feature not in NUM_STEPS:
        raise SystemExit("%s is not a supported feature." % feature)
    if a.gene_pattern is not None and a.gene_annotations is not None:
        raise SystemExit("At most one of --gene-pattern and --gene-annotations can be given.")
    if a.kallisto and a.kallisto_bootstrap:
        raise SystemExit("Only one of '--kallisto' and '--kallisto-bootstrap' can be used.")
    use_kallisto = a.kallisto or a.kallisto_bootstrap
    if use_kallisto and a.point_estimates is not None:
        raise SystemExit("'--use-point-estimates' in not compatible with '--kallisto' or '--kallisto-bootstrap'")
    point = use_kallisto or a.point_estimates is not None
    if a.pseudocount is not None and not point:
        raise SystemExit("--pseudocount argument only valid with --point-estimates")
    if feature != "transcript" and a.kallisto_bootstrap:
        raise SystemExit("%s regression with --kallisto-bootstrap not yet implemented" % feature)
    if feature != "transcript" and point:
        raise SystemExit("%s regression is built on the approximate likelihood only: --point-estimates and --kallisto need "
                         "--feature transcript" % feature)
    if feature != "transcript" and a.gene_pattern is None and a.gene_annotations is None:
        raise SystemExit("--feature %s needs --gene-pattern or --gene-annotations (GFF parsing is not built, DESIGN.md section 7)" % feature)
    if a.point_estimates is not None and not a.transcript_ids:
        raise SystemExit("--point-estimates needs --transcript-ids: the CSV rows are matched by transcript id")
    num_steps = NUM_STEPS[feature] if a.num_steps is None else a.num_steps
    if num_steps < 1 or a.effect_draws < 1:
        raise SystemExit("--num-steps and --effect-draws must be positive")
    if a.effect_draws > MAX_EFFECT_DRAWS:
        raise SystemExit("--effect-draws: the effect-size kernel is built for at most %d draws" % MAX_EFFECT_DRAWS)
    from . import estimate, h5io
    from .core import Context
    from .pca import read_experiment
    from .sample import _read_lines, resolve_names
    spec = read_experiment(a.experiment)
    if not spec.get("samples"):
        raise SystemExit("%s names no samples" % a.experiment)
    ids_given = _read_lines(a.transcript_ids) if a.transcript_ids else None
    ctx = Context(a.device)
    pseudocount = 0.0 if a.pseudocount is None else a.pseudocount
    log_x0_std, variables = None, None
    if use_kallisto:
        _, sample_names, sample_factors = estimate.read_specification(spec)
        x0, log_x0_std = load_kallisto_estimates([s["kallisto"] for s in spec["samples"]], pseudocount, a.kallisto_bootstrap, ids_given)
    elif a.point_estimates is not None:
        from .classify import load_point_estimates
        filenames, sample_names, sample_factors = estimate.read_specification(spec, point_estimates_key=a.point_estimates)
        x0 = load_point_estimates(filenames, ids_given)
        x0 = (x0 + np.float32(pseudocount / np.float32(1e6))).astype(np.float32)  # (:228-230: added whenever the mode is on)
    else:
        filenames, _, _ = estimate.read_specification(spec)
        n = h5io.read_prepared_sample(filenames[0])["n"]
        ls = estimate.load_samples_from_specification(spec, n, ptt_filename=a.transformation, ctx=ctx)
        x0, sample_names, sample_factors, variables = ls.x0_values, ls.sample_names, ls.sample_factors, ls.variables["approx"]
    num_samples, n = x0.shape
    ids, _ = resolve_names(n, ids_given)
    with np.errstate(divide="ignore"):
        x0_log = np.log(x0).astype(np.float32)
    if point and not np.isfinite(x0_log).all():
        raise SystemExit("a point estimate of 0 has log -inf: give --pseudocount C")
    F, factor_names = build_design_matrix(sample_factors, None if a.factors is None else a.factors.split(","),
                                          a.redundant_factor if a.nonredundant else None, a.balanced)
    if F.shape[1] < 1:
        raise SystemExit("the design matrix has no columns: the samples name no factors (or --nonredundant removed them all)")
    distortion = not a.no_distortion
    if feature == "transcript":
        sample_scales = estimate_sample_scales(x0_log)
        if log_x0_std is not None:
            reg = RNASeqNormalTranscriptLinearRegression(None, x0_log, log_x0_std, F, sample_scales, distortion, a.scale_penalty, ctx=ctx)
        else:
            reg = RNASeqTranscriptLinearRegression(variables, x0_log, F, sample_scales, distortion, a.scale_penalty, point, ctx=ctx)
        qx_loc, qw_loc, qw_scale, qx_bias, qx_scale = reg.fit(num_steps, seed=a.seed)
        feature_names, feature_names_label = ids, "transcript_id"
    else:
        annotations = None if a.gene_annotations is None else read_experiment(a.gene_annotations)
        num_features, gene_idxs, transcript_idxs, gene_ids, gene_names = gene_map(ids, a.gene_pattern, annotations)
        gene_sizes = np.bincount(gene_idxs - 1, minlength=num_features).astype(np.float32)
        x_gene_init, x_isoform_init = gene_initial_values(gene_idxs, transcript_idxs, x0, num_samples, num_features, n)
        sample_scales = estimate_sample_scales(x0_log, upper_quantile=0.95)
        if feature == "gene":
            reg = RNASeqGeneLinearRegression(variables, gene_idxs, transcript_idxs, x_gene_init, x_isoform_init, gene_sizes, F,
                                             sample_scales, distortion, a.scale_penalty, False, ctx=ctx)
            qx_loc, qw_loc, qw_scale, qx_bias, qx_scale = reg.fit(num_steps, seed=a.seed)
            feature_names, feature_names_label = gene_ids, "gene_id"
        else:
            if a.x_isoform_init_output is not None:
                write_x_init(a.x_isoform_init_output, "transcript_id", ids, x_isoform_init)
            if a.x_gene_init_output is not None:
                write_x_init(a.x_gene_init_output, "gene_id", gene_ids, x_gene_init)
            reg = RNASeqGeneIsoformLinearRegression(variables, gene_idxs, transcript_idxs, x_gene_init, x_isoform_init, gene_sizes, F, F,
                                                    sample_scales, distortion, a.scale_penalty, False, ctx=ctx)
            (qw_loc, qw_scale, qw_isoform_loc, qw_isoform_scale, qx_isoform_bias_loc, qx_isoform_bias_scale, qx_isoform_scale,
             qx_bias, qx_scale, qx_gene_loc_factor_est) = reg.fit(num_steps, seed=a.seed)
            # (the reference leaves qx_loc undefined on this branch and fails at --output-expression: the genes' qx_loc is written)
            qx_loc = reg.variables()["qx_loc"] if a.output_expression is not None else None
            print("estimating effect sizes...")
            # (the reference dies in log(abs(nothing)) without --isoform-effect-size; here prob_de is then not computed)
            es = None if a.isoform_effect_size is None else math.log(abs(a.isoform_effect_size))
            min_es, mean_es, prob_de, a_min, a_mean, a_prob = estimate_isoform_effect_sizes(
                gene_idxs, transcript_idxs, es, a.aitchison_distance_effect_size, qw_isoform_loc, qw_isoform_scale, qx_isoform_bias_loc,
                qx_isoform_bias_scale, qx_gene_loc_factor_est, niter=a.effect_draws, target_coverage=a.min_effect_size_coverage,
                seed=a.seed, ctx=ctx)
            print("done.")
            if a.aitchison_distance_output is not None:
                write_aitchison_results(a.aitchison_distance_output, factor_names, gene_ids, gene_names, a_min, a_mean, a_prob)
            write_isoform_regression_effects(a.isoform_output, gene_idxs, transcript_idxs, factor_names, gene_ids, gene_names, ids,
                                             min_es, mean_es, prob_de, qw_isoform_loc, qx_isoform_bias_loc, qx_isoform_scale)
            if a.extra_params_output is not None:
                reg.write_other_params(a.extra_params_output)
            feature_names = ["%s,%s" % gn for gn in zip(gene_ids, gene_names)]
            feature_names_label = "gene_id,gene_name"
    if a.output_expression is not None:
        write_expression(a.output_expression, feature_names_label, feature_names, sample_names, qx_loc)
    write_regression_effects(a.output, factor_names, feature_names_label, feature_names, qx_bias, qx_scale, qw_loc, qw_scale,
                             a.lower_credible, a.upper_credible, a.effect_size, a.min_effect_size_coverage,
                             a.write_variational_posterior_params)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())

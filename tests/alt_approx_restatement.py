"""NumPy restatement of the reference's alternative likelihood approximations, line by line: logistic_normal, normal_ilr and
normal_alr of src/likelihood-approximation-alt.jl with src/isometric_log_ratios.jl, src/additive_log_ratios.jl, ADAM of
src/likelihood-approximation.jl:107-146 and sample_likap of src/evaluate.jl.  Everything is Float64 unless `f32=True`, which keeps
Float32 where the reference does (xs, y_grad, the gradient accumulators, x_grad for ILR and ALR, sigma, the parameters' moments):
the reference's own arithmetic, used to show that the parity bounds can be met by it.  xs handed to the likelihood is Float32
in both modes (the reference's array type, and what the sparse pass takes).  `log_likelihood` is a callable xs f32[n] ->
(lp, x_grad f64[n]), e.g. oracle.Sample(...).log_likelihood.

Quirks restated as written, not as one would derive them:
  - logistic_normal :148-160: xsum is taken after normalisation (and clamping), in ln_ladj and in its gradient; ln_ladj is not
    the transform's log-determinant (tests/test_alt_approx_host.py);
  - additive_log_ratios.jl:27, 69: alr_ladj lacks (n - 1) log(1 + sum exp ys) of the log-determinant; `1 - xs[i]` is its gradient,
    taken with the clamped xs;
  - isometric_log_ratios.jl:98,108: `dladj_dxi = 1 / xs[i]`, added to x_grad before the normalisation's chain rule;
  - logistic_normal: `elbo = lp + ln_ladj` is an assignment in the draw loop (:162), so elbo is the LAST draw's value over K;
    ILR and ALR accumulate (:579, 698);
  - logistic_normal's initial omega is 0.1, not log(0.1) (:79)."""
import numpy as np

METHODS = ("logistic_normal", "normal_ilr", "normal_alr")
EPS = 1e-10

# constants.jl:48-65
ADAM_INITIAL_LEARNING_RATE, ADAM_LEARNING_RATE_DECAY, ADAM_MIN_LEARNING_RATE = 1.0, 2e-2, 1e-3
ADAM_EPS, ADAM_RV, ADAM_RM = 1e-8, 0.9, 0.7


# ---- the tree (hclust.jl:392-414 deserialize_tree) -----------------------------------------------------------------------------
class Tree:
    """nodes in DFS pre-order, right child first: the FIRST child met of a node is its right child (hclust.jl:403-408)"""

    def __init__(self, node_parent_idxs, node_js):
        p = np.asarray(node_parent_idxs, np.int64)
        self.js = np.asarray(node_js, np.int64)
        N = len(p)
        self.N, self.n = N, (N + 1) // 2
        self.left = np.full(N, -1, np.int64)
        self.right = np.full(N, -1, np.int64)
        for i in range(1, N):
            par = p[i] - 1
            if self.right[par] < 0:
                self.right[par] = i
            else:
                self.left[par] = i
        self.size = np.ones(N, np.int64)  # set_subtree_sizes!
        for i in range(N - 1, -1, -1):
            if self.js[i] == 0:
                self.size[i] = self.size[self.left[i]] + self.size[self.right[i]]
        self.internal = np.flatnonzero(self.js == 0)  # k-th internal node in node order

    def coefficients(self):
        """a, b of every internal node (isometric_log_ratios.jl:62-66), and r, s"""
        r = self.size[self.left[self.internal]].astype(np.float64)
        s = self.size[self.right[self.internal]].astype(np.float64)
        return np.sqrt(s / (r * (r + s))), -np.sqrt(r / (s * (r + s))), r.astype(np.int64), s.astype(np.int64)


def _clamp_f32(xs):
    """clamp!(xs::Vector{Float32}, eps, 1 - eps): the bounds are converted to Float32 (1 - 1e-10 becomes 1)"""
    return np.clip(xs.astype(np.float32), np.float32(EPS), np.float32(1 - EPS))


# ---- isometric_log_ratios.jl ---------------------------------------------------------------------------------------------------
def ilr_transform(t, ys, f32=False):
    """ilr_transform! (:43-86) -> xs (normalised, unclamped), ladj of the unclamped xs, state for the gradients"""
    a, b, _, _ = t.coefficients()
    val = np.zeros(t.N, np.float64)  # input_value (Float32 fields in the reference's node; the yardstick keeps f64)
    xs = np.zeros(t.n, np.float32 if f32 else np.float64)
    k = 0
    for i in range(t.N):
        if t.js[i] != 0:
            xs[t.js[i] - 1] = np.exp(val[i])
            continue
        val[t.left[i]] = a[k] * ys[k] + val[i]
        val[t.right[i]] = b[k] * ys[k] + val[i]
        if f32:
            val[t.left[i]], val[t.right[i]] = np.float32(val[t.left[i]]), np.float32(val[t.right[i]])
        k += 1
    xs_sum = float(xs.sum(dtype=np.float64))
    xs = xs / xs.dtype.type(xs_sum)
    ladj = float(np.log(xs.astype(np.float64)).sum() + np.log(np.sqrt(t.n)))
    return xs, ladj, (val, xs_sum)


def ilr_transform_gradients(t, xs, x_grad, state, f32=False):
    """ilr_transform_gradients! (:91-128); xs: the CLAMPED values the fit passes in (likelihood-approximation-alt.jl:575, 581)"""
    val, xs_sum = state
    a, b, _, _ = t.coefficients()
    xs = xs.astype(np.float64)
    c = float(np.sum(xs * (x_grad + 1.0 / xs) / xs_sum))
    grad = np.zeros(t.N, np.float32 if f32 else np.float64)
    y_grad = np.zeros(t.n - 1, np.float32 if f32 else np.float64)
    k = t.n - 2
    for i in range(t.N - 1, -1, -1):
        if t.js[i] != 0:
            j = t.js[i] - 1
            g = (1 / xs_sum) * (x_grad[j] + 1.0 / xs[j]) - c
            grad[i] = np.exp(val[i]) * g
        else:
            lg, rg = grad[t.left[i]], grad[t.right[i]]
            grad[i] = lg + rg
            y_grad[k] = a[k] * lg + b[k] * rg
            k -= 1
    assert k == -1
    return y_grad


def ilr_ygrad_terms(t, xs, x_grad, state):
    """T of the GPU test's y_grad bound: |a| sum_left |l| + |b| sum_right |l| over the leaf gradients l"""
    val, xs_sum = state
    a, b, _, _ = t.coefficients()
    xs = xs.astype(np.float64)
    c = float(np.sum(xs * (x_grad + 1.0 / xs) / xs_sum))
    mag = np.zeros(t.N)
    T = np.zeros(t.n - 1)
    k = t.n - 2
    for i in range(t.N - 1, -1, -1):
        if t.js[i] != 0:
            j = t.js[i] - 1
            mag[i] = abs(np.exp(val[i]) * ((1 / xs_sum) * (x_grad[j] + 1.0 / xs[j]) - c))
        else:
            mag[i] = mag[t.left[i]] + mag[t.right[i]]
            T[k] = abs(a[k]) * mag[t.left[i]] + abs(b[k]) * mag[t.right[i]]
            k -= 1
    return T


# ---- additive_log_ratios.jl ----------------------------------------------------------------------------------------------------
def alr_transform(refidx, ys, f32=False):
    """alr_transform! (:12-31), refidx 1-based"""
    n = len(ys) + 1
    eta = np.insert(np.asarray(ys, np.float64), refidx - 1, 0.0)
    xs = np.exp(eta).astype(np.float32 if f32 else np.float64)
    xs = xs / xs.sum()
    ladj = float(np.sum(ys, dtype=np.float64) - np.log(1 + np.sum(np.exp(np.asarray(ys, np.float64)))))
    assert len(xs) == n
    return xs, ladj


def alr_transform_gradients(refidx, xs, x_grad, f32=False):
    """alr_transform_gradients! (:49-71); xs: the clamped values"""
    xs = xs.astype(np.float64)
    c = float(np.sum(xs * x_grad))
    keep = np.arange(len(xs)) != refidx - 1
    y_grad = (xs * x_grad - xs * c + (1 - xs))[keep]
    return y_grad.astype(np.float32) if f32 else y_grad


# ---- likelihood-approximation-alt.jl:138-160 -----------------------------------------------------------------------------------
def logistic_normal_gradients(xs, x_grad):
    """xs: the clamped values, f64 [n] -> (y_grad [n-1], ln_ladj), as written"""
    n = len(xs)
    c = float(np.sum(xs * x_grad))
    y_grad = xs[:-1] * x_grad[:-1] - xs[:-1] * c
    xsum = float(xs[:-1].sum())  # after normalisation
    y_grad = y_grad + (1 / (1 + xsum)) * (xs[:-1] - xs[:-1] * xsum) + 1 - xs[:-1] * (n - 1)
    return y_grad, float(np.log(1 + xsum) + np.log(xs[:-1]).sum())


# ---- one draw of each method ---------------------------------------------------------------------------------------------------
def draw(method, log_likelihood, mu, sigma, zs, tree=None, refidx=None, f32=False):
    """The body of the draw loop -> dict(xs f32 clamped, x_grad, y_grad, lp, ladj, terms)."""
    n = len(mu) + 1
    F = np.float32
    # ys = zs * sigma + mu: Float32 operands, so a Float32 product and sum in the reference whatever the array they land in
    ys = (F(1) * zs.astype(F) * sigma.astype(F) + mu.astype(F)).astype(np.float64)
    out = {}
    if method == "logistic_normal":  # likelihood-approximation-alt.jl:116-172
        ex = np.append(np.exp(ys), 1.0)
        if f32:
            ex = ex.astype(F)
            s = F(1)
            for v in ex[:-1]:
                s = F(s + v)  # exp_y_sum += xs[i]
            xs = ex / s
        else:
            xs = ex / ex.sum()
        xs = _clamp_f32(xs)
        lp, x_grad = log_likelihood(xs)
        x64 = xs.astype(np.float64)
        y_grad, ladj = logistic_normal_gradients(x64, x_grad)
        c = float(np.sum(x64 * x_grad))
        out["terms"] = np.abs(x64[:-1] * x_grad[:-1]) + np.abs(x64[:-1] * c) + 1 + np.abs(x64[:-1] * (n - 1))
    elif method == "normal_ilr":  # :569-581
        xs_u, ladj_u, state = ilr_transform(tree, ys, f32)
        xs = _clamp_f32(xs_u)
        # (ilr_ladj is computed inside ilr_transform!, before the clamp of :575)
        ladj = ladj_u
        lp, x_grad = log_likelihood(xs)
        if f32:
            x_grad = x_grad.astype(F).astype(np.float64)  # x_grad = Array{Float32} (:545)
        y_grad = ilr_transform_gradients(tree, xs, x_grad, state, f32)
        out["terms"] = ilr_ygrad_terms(tree, xs, x_grad, state)
    elif method == "normal_alr":  # :688-700
        xs_u, ladj = alr_transform(refidx, ys, f32)
        xs = _clamp_f32(xs_u)
        lp, x_grad = log_likelihood(xs)
        if f32:
            x_grad = x_grad.astype(F).astype(np.float64)
        y_grad = alr_transform_gradients(refidx, xs, x_grad, f32)
        x64 = np.delete(xs.astype(np.float64), refidx - 1)
        g = np.delete(x_grad, refidx - 1)
        out["terms"] = np.abs(x64 * g) + np.abs(x64 * float(np.sum(xs.astype(np.float64) * x_grad))) + 1
    else:
        raise ValueError(method)
    if f32:
        y_grad = y_grad.astype(F)
    out.update(xs=xs, x_grad=x_grad, y_grad=y_grad, lp=float(lp), ladj=ladj, ys=ys)
    return out


def step_gradients(method, log_likelihood, mu, omega, zs, tree=None, refidx=None, f32=False):
    """One step's K draws -> the draws and the averaged parameter gradients (:111-178)."""
    F = np.float32 if f32 else np.float64
    sigma = np.exp(omega.astype(np.float32)) if f32 else np.exp(omega.astype(np.float64))
    K = len(zs)
    mu_grad = np.zeros(len(mu), F)
    omega_grad = np.zeros(len(mu), F)
    draws = []
    for d in range(K):
        r = draw(method, log_likelihood, mu, sigma, zs[d], tree, refidx, f32)
        yg = r["y_grad"].astype(F)
        mu_grad += yg
        sigma_grad = zs[d].astype(F) * yg
        omega_grad += sigma.astype(F) * sigma_grad
        draws.append(r)
    mu_grad /= F(K)
    omega_grad /= F(K)
    if method == "logistic_normal":
        elbo = (draws[-1]["lp"] + draws[-1]["ladj"]) / K
    else:
        elbo = sum(r["lp"] + r["ladj"] for r in draws) / K
    return dict(draws=draws, mu_grad=mu_grad, omega_grad=omega_grad, elbo=elbo, lp_mean=sum(r["lp"] for r in draws) / K)


# ---- ADAM (likelihood-approximation.jl:107-146) --------------------------------------------------------------------------------
def adam_learning_rate(step_num):
    return max(ADAM_MIN_LEARNING_RATE, ADAM_INITIAL_LEARNING_RATE * np.exp(-ADAM_LEARNING_RATE_DECAY * step_num))


def adam_update(params, ms, vs, grad, step_num, max_step_size):
    """adam_update_mv! + adam_update_params!; params, ms, vs are Float32 arrays in the reference"""
    g = grad.astype(np.float64)
    if step_num == 1:
        ms[:] = g
        vs[:] = g * g
    else:
        ms[:] = ADAM_RM * ms.astype(np.float64) + (1 - ADAM_RM) * g
        vs[:] = ADAM_RV * vs.astype(np.float64) + (1 - ADAM_RV) * g * g
    lr = adam_learning_rate(step_num - 1)
    pm = ms.astype(np.float64) / (1 - ADAM_RM ** step_num)
    pv = vs.astype(np.float64) / (1 - ADAM_RV ** step_num)
    delta = lr * pm / (np.sqrt(pv) + ADAM_EPS)
    params[:] = params.astype(np.float64) + np.clip(delta, -max_step_size, max_step_size)


def initial_params(method, n):
    mu = np.zeros(n - 1, np.float32)
    omega = np.full(n - 1, np.float32(0.1) if method == "logistic_normal" else np.log(np.float32(0.1)), np.float32)
    return mu, omega


def max_step(method):
    return 2e-2 if method == "logistic_normal" else 2e-1


def fit(method, log_likelihood, n, z0, tree=None, refidx=None, f32=False):
    """approximate_likelihood of `method` with supplied noise z0 [steps][K][n-1] -> dict(mu, omega, elbo, lp_mean)."""
    mu, omega = initial_params(method, n)
    m_mu, v_mu, m_om, v_om = (np.zeros(n - 1, np.float32) for _ in range(4))
    elbo, lp_mean = [], []
    for step_num in range(1, len(z0) + 1):
        r = step_gradients(method, log_likelihood, mu, omega, z0[step_num - 1], tree, refidx, f32)
        assert np.isfinite(r["elbo"])
        elbo.append(r["elbo"])
        lp_mean.append(r["lp_mean"])
        adam_update(mu, m_mu, v_mu, r["mu_grad"], step_num, max_step(method))
        adam_update(omega, m_om, v_om, r["omega_grad"], step_num, max_step(method))
    return dict(mu=mu, omega=omega, elbo=np.array(elbo), lp_mean=np.array(lp_mean))


# ---- evaluate.jl:34-74, 203-275 ------------------------------------------------------------------------------------------------
def sample_likap(method, mu, omega, efflens, zs, tree=None, refidx=None):
    """`len(zs)` draws, each divided by the effective lengths and renormalised"""
    sigma = np.exp(omega.astype(np.float32))
    out = np.empty((len(zs), len(mu) + 1), np.float64)
    for i, z in enumerate(zs):
        ys = (z.astype(np.float32) * sigma + mu.astype(np.float32)).astype(np.float64)
        if method == "logistic_normal":
            ex = np.append(np.exp(ys), 1.0)
            xs = ex / ex.sum()
        elif method == "normal_ilr":
            xs = ilr_transform(tree, ys)[0]
        else:
            xs = alr_transform(refidx, ys)[0]
        xs = _clamp_f32(xs).astype(np.float64) / efflens.astype(np.float64)
        out[i] = xs / xs.sum()
    return out


# ---- change of variables, for the host tests -----------------------------------------------------------------------------------
def forward(method, ys, tree=None, refidx=None):
    """ys -> (xs unclamped f64, ladj) of the transform alone"""
    ys = np.asarray(ys, np.float64)
    if method == "normal_ilr":
        xs, ladj, _ = ilr_transform(tree, ys)
        return xs, ladj
    if method == "normal_alr":
        return alr_transform(refidx, ys)
    ex = np.append(np.exp(ys), 1.0)
    xs = ex / ex.sum()
    return xs, float(np.log(1 + xs[:-1].sum()) + np.log(xs[:-1]).sum())

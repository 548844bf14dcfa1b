"""Plain NumPy float64 restatement of the density of the fitted likelihood approximation, RNASeqApproxLikelihoodDist._log_prob
(src/polee_approx_likelihood.py:367-450), and of its gradient through InvHSB's registered backward pass (hsb_ops.cpp:342-391 as
oracle/polee_oracle.c:279-315 and :984-1072 restate it) -- what tests/test_gpu_approx_density.py holds polee_amd/csrc/approx.hip to,
node by node.  A helper module, not a test file.  It also holds the inputs of those tests (CASES, inputs), the tolerances measured
from the restatement alone (G_NODE, G_GRAD, T_NODE, T_GRAD) and three CPU-only mutants (tests/test_approx_density_host.py).

Per sample, with p = softmax(x), r = p * efflen, q = r / sum r:
    u      subtree sums of q, BOTTOM-UP (sums of positive numbers: no prefix differences, nothing cancels)
    y      u_left / u per internal node; y_logit = log y - log1p(-y); z_std = (y_logit - mu) / sigma; z = sinh(asinh(z_std) - alpha)
    lp     sum over nodes of [-log u - log y - log1p(-y) - log sigma + log cosh(alpha - asinh z_std) - log1p(z_std^2) / 2
           - (log 2 pi + z^2) / 2]  +  sum x - (n-1) log sum exp x + sum log efflen - log sum r
    y_grad d lp / d y of every node; the node's two tour terms (what InvHSBGrad adds on the way down to either child)
               tp0 = -1/u - y/u y_grad      (edge to the RIGHT child)
               tp1 = -1/u + (1-y)/u y_grad  (edge to the LEFT child, the one y multiplies)
    bp_j   the sum of the tour terms over leaf j's ancestors (d lp / d q_j); path_abs_j the sum of their magnitudes
    x_grad p (g_p - <g_p, p>) + 1 - (n-1) p with g_p = ((bp - <bp,q>) - 1) efflen / sum r

f32_steps=True rounds to float32 where the oracle (and the reference's TensorFlow graph) does: exp(x), p, r and q, log efflen,
y_logit, the -log y - log1p(-y) term, z_std, log sigma, asinh, z, the log-cosh term, and bp where it enters <bp, q>.  Two things the
oracle does are NOT restated, in either mode: InvHSB's running Float32 accumulator of -log u (its error depends on the order of
the nodes alone and is hundreds of ulps of lp at these sizes; the sum here is exact), and InvHSBGrad's top-down recomputation of u
from y with u_root = 1 (u here is the bottom-up sum the forward pass made y from).  f32_steps=False keeps every step in float64.

Nodes are identified across implementations by (smallest transcript of the subtree, number of leaves), which is unique in a tree.
"""
import functools
import math

import numpy as np

from conftest import random_tree

F64 = np.float64
CHUNK = 512  # leaves per chunk of the device's leaf pass (mutant (c) and the choice of shapes; the restatement itself has no chunks)


class Tree:
    """A serialised tree (node_parent_idxs, node_js; parents precede children, the first child listed is the RIGHT one:
    src/ptt.jl:293-309) as child arrays, with the internal nodes numbered k = 0.. in array order."""

    def __init__(self, parents, js):
        parents, js = np.asarray(parents, np.int64), np.asarray(js, np.int64)
        N = len(parents)
        self.N, self.n = N, (N + 1) // 2
        self.left, self.right = np.full(N, -1, np.int64), np.full(N, -1, np.int64)
        for i in range(1, N):
            p = parents[i] - 1
            assert 0 <= p < i
            if self.right[p] < 0:
                self.right[p] = i
            else:
                assert self.left[p] < 0
                self.left[p] = i
        self.leaf = js - 1  # 0-based transcript, -1 for internal nodes
        self.nodes = np.flatnonzero(self.leaf < 0)  # k -> node
        assert len(self.nodes) == self.n - 1 and (self.left[self.nodes] > 0).all() and (self.right[self.nodes] > 0).all()
        # sizes and smallest transcripts bottom-up, leaf positions (right subtree first) top-down
        size, mn = np.ones(N, np.int64), np.where(self.leaf >= 0, self.leaf, N)
        for j in self.nodes[::-1]:
            l, r = self.left[j], self.right[j]
            size[j] = size[l] + size[r]
            mn[j] = min(mn[l], mn[r])
        lo = np.zeros(N, np.int64)
        for j in self.nodes:
            lo[self.right[j]] = lo[j]
            lo[self.left[j]] = lo[j] + size[self.right[j]]
        self.size, self.min_tid, self.pos_lo = size, mn, lo
        self.k_size, self.k_min_tid = size[self.nodes], mn[self.nodes]
        self.k_size_right, self.k_size_left = size[self.right[self.nodes]], size[self.left[self.nodes]]
        self.k_lo = lo[self.nodes]
        self.k_mid = self.k_lo + self.k_size_right
        self.k_hi = self.k_lo + self.k_size
        self.leaf_order = np.empty(self.n, np.int64)  # leaf position -> transcript
        lf = np.flatnonzero(self.leaf >= 0)
        self.leaf_order[lo[lf]] = self.leaf[lf]

    def index_arrays(self):
        """left_index, right_index, leaf_index as the reference passes them (0-based, -1 = none)"""
        return self.left.astype(np.int32), self.right.astype(np.int32), self.leaf.astype(np.int32)

    def sums(self, q):
        """(u_left, u_right) per internal node: subtree sums bottom-up"""
        u = np.zeros(self.N, F64)
        lf = self.leaf >= 0
        u[lf] = q[self.leaf[lf]]
        for j in self.nodes[::-1]:
            u[j] = u[self.left[j]] + u[self.right[j]]
        return u[self.left[self.nodes]], u[self.right[self.nodes]]

    def push_down(self, t_left, t_right):
        """per transcript: the sum over the leaf's ancestors of the term of the edge taken"""
        v = np.zeros(self.N, F64)
        for k, j in enumerate(self.nodes):
            v[self.left[j]] = v[j] + t_left[k]
            v[self.right[j]] = v[j] + t_right[k]
        out = np.empty(self.n, F64)
        lf = self.leaf >= 0
        out[self.leaf[lf]] = v[lf]
        return out


def _fsum(a):
    return math.fsum(np.asarray(a, F64).ravel().tolist())


def leaf_masses(x, eff, f32_steps):
    """q (as float64 values) and what the outer terms of lp need, of one sample"""
    F = np.float32 if f32_steps else F64
    x, l = np.asarray(x, np.float32), np.asarray(eff, np.float32)
    ex = np.exp(x.astype(F)).astype(F64)  # :379
    sum_exp = _fsum(ex)
    p = (ex / sum_exp).astype(F)  # :387
    r = p * l.astype(F)  # :395
    R = _fsum(r)
    q = (r.astype(F64) / R).astype(F).astype(F64)  # :397
    outer = _fsum(x) - (len(x) - 1) * math.log(sum_exp) + _fsum(np.log(l.astype(F))) - math.log(R)  # :384, :390, :399-400
    return q, ex / sum_exp, R, outer


def density(tree, x, eff, mu, sigma, alpha, f32_steps=True, sums=None, tour_prefix=False):
    """One sample.  sums: replaces Tree.sums (mutants (a), (c)); tour_prefix: bp by mutant (b)'s running prefix."""
    F = np.float32 if f32_steps else F64
    n = tree.n
    q, p, R, outer = leaf_masses(x, eff, f32_steps)
    ul, ur = (sums or Tree.sums)(tree, q)
    with np.errstate(all="ignore"):  # (a mutant may hand over sums that are not positive)
        u = ul + ur
        y = ul / u  # hsb_ops.cpp:230
        y_log, y_1mlog = np.log(y), np.log1p(-y)  # :418-419
        y_logit = (y_log - y_1mlog).astype(F)  # :421
        t_y = (-y_log - y_1mlog).astype(F)  # :423-425
        mu, sg, al = (np.asarray(a, np.float32).astype(F) for a in (mu, sigma, alpha))
        z_std = (y_logit - mu) / sg  # :430
        t_sg = -np.log(sg)  # :432
        z_asinh = np.arcsinh(z_std)  # :437
        z = np.sinh(z_asinh - al)  # :438
        t_sa = np.log(np.cosh(al - z_asinh)) - F(0.5) * np.log1p(z_std * z_std)  # :440-443
        node_lp = (-np.log(u) + t_y.astype(F64) + t_sg.astype(F64) + t_sa.astype(F64)
                   + (-math.log(2.0 * math.pi) - (z * z).astype(F64)) / 2.0)  # hsb_ops.cpp:231, :448
        lp = outer + _fsum(node_lp)
        # d (lp + ladj) / d y_logit from the (rounded) z_std and alpha, in float64 (oracle :1034-1042), then d / d y
        zs, a, s64 = z_std.astype(F64), al.astype(F64), sg.astype(F64)
        c = np.arcsinh(zs) - a
        rt = np.sqrt(1.0 + zs * zs)
        d_lp = -np.sinh(c) * np.cosh(c) / rt
        d_la = np.tanh(c) / rt - zs / (1.0 + zs * zs)
        y_grad = (d_lp + d_la) / s64 / (y * (1.0 - y)) + (1.0 / (1.0 - y) - 1.0 / y)
        tp0 = -1.0 / u - y / u * y_grad
        tp1 = -1.0 / u + (1.0 - y) / u * y_grad
        bp = bp_by_tour_prefix(tree, tp0, tp1) if tour_prefix else tree.push_down(tp1, tp0)
        path_abs = tree.push_down(np.abs(tp1), np.abs(tp0))
        # chain through q = r / R, r = p l, p = softmax(x) (oracle :1049-1067); backprops is Float32 (hsb_ops.cpp:260)
        bpr = bp.astype(F).astype(F64)
        dot = _fsum(bpr * q)
        gp = ((bpr - dot) / R - 1.0 / R) * np.asarray(eff, np.float32).astype(F64)
        x_grad = p * (gp - _fsum(gp * p)) + 1.0 - (n - 1) * p
    return dict(lp=lp, x_grad=x_grad, u=u, y=y, y_grad=y_grad, tp0=tp0, tp1=tp1, bp=bp, path_abs=path_abs, q=q, p=p, dot=dot,
                node_lp=node_lp, z=z.astype(F64))


def node_scale(r):
    """what an error of a node's tour terms is measured in: (1 + |y_grad|) / u"""
    return (1.0 + np.abs(r["y_grad"])) / r["u"]


def grad_scale(r, n):
    """what an error of x_grad is measured in: q (|bp| + |<bp,q>| + 1) + 1 + (n-2) p, element by element"""
    return r["q"] * (np.abs(r["bp"]) + abs(r["dot"]) + 1.0) + 1.0 + (n - 2) * r["p"]


def ulp32(v):
    """one Float32 ulp at |v|"""
    return np.spacing(np.abs(np.asarray(v, F64)).astype(np.float32)).astype(F64)


# ---- mutants: three ways an implementation goes wrong that the public outputs (lp as Float32, x_grad = q * ...) do not show ----

def sums_from_plain_prefix(tree, q):
    """(a) node sums as differences of ONE plain-double prefix of q over the leaf order: a double-double prefix whose low word
    is lost"""
    C = np.concatenate([[0.0], np.cumsum(q[tree.leaf_order])])
    return C[tree.k_hi] - C[tree.k_mid], C[tree.k_mid] - C[tree.k_lo]


def bp_by_tour_prefix(tree, tp0, tp1):
    """(b) bp as a plain-double running prefix over the whole Euler tour, +term entering an edge and -term leaving it: the
    three-phase scan without its double-double accumulator (the terms of tiny subtrees stay behind as rounding residue)"""
    k_of = np.full(tree.N, -1, np.int64)
    k_of[tree.nodes] = np.arange(tree.n - 1)
    out = np.empty(tree.n, F64)
    run = 0.0
    stack = [(0, 0.0, True)]
    while stack:
        j, t, enter = stack.pop()
        if not enter:
            run -= t
            continue
        run += t
        stack.append((j, t, False))
        if tree.leaf[j] >= 0:
            out[tree.leaf[j]] = run
        else:
            k = k_of[j]
            stack.append((int(tree.left[j]), float(tp1[k]), True))
            stack.append((int(tree.right[j]), float(tp0[k]), True))  # (popped first: right child first)
    return out


def crossing_nodes(tree):
    """the internal nodes whose leaf range does not lie in one chunk of CHUNK leaf positions"""
    return np.flatnonzero((tree.k_hi - 1) // CHUNK != tree.k_lo // CHUNK)


def sums_one_offset_lost(tree, q):
    """(c) the middle one of the tree's crossing nodes takes its upper boundary from the chunk-local prefix, without the sum of
    the chunks before it"""
    ul, ur = tree.sums(q)
    cr = crossing_nodes(tree)
    k = cr[len(cr) // 2]
    ql = q[tree.leaf_order]
    first = (tree.k_hi[k] - 1) // CHUNK * CHUNK  # first position of the chunk the node ends in
    ul = ul.copy()
    ul[k] -= ql[:first].sum()
    return ul, ur


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def _serialise(t):
    """nested (left, right) tuples of 1-based transcripts -> (node_parent_idxs, node_js), DFS pre-order, right child first"""
    parents, js = [], []
    stack = [(t, 0)]
    while stack:
        node, par = stack.pop()
        idx = len(parents) + 1
        parents.append(par)
        if isinstance(node, tuple):
            js.append(0)
            stack.append((node[0], idx))
            stack.append((node[1], idx))
        else:
            js.append(int(node))
    return np.array(parents, np.int32), np.array(js, np.int32)


def one_sided_caterpillar(n, rng, leaf_first):
    """A caterpillar whose leaves all hang on the same side.  leaf_first=False: the spine is every node's right child, so every
    node's leaf range starts at position 0; True: the mirror image, every node's range ends at n."""
    perm = list(rng.permutation(n) + 1)
    t = perm[0]
    for j in perm[1:]:
        t = (t, j) if leaf_first else (j, t)
    return _serialise(t)


def _make_tree(kind, n, rng):
    if kind == "spine_lo":
        return one_sided_caterpillar(n, rng, False)
    if kind == "spine_hi":
        return one_sided_caterpillar(n, rng, True)
    return random_tree(n, rng, kind)


# name -> (n, tree kind per sample, shared tree, seed).  The seeds are the first ones for which input_conditions() holds and the
# Float32 steps move lp by less than a tenth of a Float32 ulp (tests/test_approx_density_host.py asserts both).
CASES = {
    "n2": (2, ("random",), False, 11),
    "n3": (3, ("random",), False, 3),
    "random511": (511, ("random",), False, 1),
    "random512": (512, ("random",), False, 1),
    "random513": (513, ("random",), False, 1),
    "balanced1024": (1024, ("balanced",), False, 7),
    "balanced2048": (2048, ("balanced",), False, 2),
    "spine1100": (1100, ("spine",), False, 1),
    "spine3000": (3000, ("spine",), False, 1),
    "random3000": (3000, ("random",), False, 1),
    "spine_lo1537": (1537, ("spine_lo",), False, 1),
    "spine_hi1537": (1537, ("spine_hi",), False, 1),
    "mixed1536": (1536, ("spine", "balanced", "random"), False, 1),
    "shared1536": (1536, ("random",) * 3, True, 1),
}
VARIANT_CASES = ("random513", "balanced1024", "spine1100", "mixed1536")  # also run on the library's fallback paths


def _is_spine(kind):
    return kind.startswith("spine")


def centre_logits(tree, kind, rng):
    """logit0 per node: the centre of y = u_left / u.  Random and balanced trees: N(0, 3) and N(0, 3.5).  Caterpillars: +-c towards
    the larger subtree plus N(0, 0.5), and forty nodes at +-18 towards it (their hanging leaf is tiny; an extreme node AGAINST the
    larger subtree would take the whole spine below Float32).  c = 5 at n = 3000, where the spine decays to some 1e-10; the smaller
    caterpillars lean less (c = logit(1 - 26 / n)), so that their spines decay as far in fewer nodes."""
    nm1 = tree.n - 1
    if not _is_spine(kind):
        return rng.normal(0.0, 3.5 if kind == "balanced" else 3.0, nm1)
    c = 5.0 if tree.n >= 3000 else math.log(tree.n / 26.0 - 1.0)
    sign = np.where(tree.k_size_left >= tree.k_size_right, 1.0, -1.0)
    lg = sign * c + rng.normal(0.0, 0.5, nm1)
    ext = rng.integers(0, nm1, 40)
    lg[ext] = sign[ext] * 18.0
    return lg


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The case's trees and arrays (read-only): x, efflen [S][n]; la_mu, la_sigma, la_alpha [S][n-1]; index arrays [S or 1][N].
    x is built from the tree -- centres pushed down in float64 to leaf masses q0, x = log(q0 / efflen) shifted to max 0 -- and
    la_mu follows the y that the Float32-rounded q gives, at sigma N(0, 1) from it: z stays O(1) as in a fitted sample, while u
    spans many decades."""
    n, kinds, shared, seed = CASES[name]
    S = len(kinds)
    rng = np.random.default_rng([seed, n])
    trees, serial = [], []
    for s in range(1 if shared else S):
        serial.append(_make_tree(kinds[s], n, rng))
        trees.append(Tree(*serial[-1]))
    x, eff = np.empty((S, n), np.float32), rng.uniform(200, 3000, size=(S, n)).astype(np.float32)
    mu = np.empty((S, n - 1), np.float32)
    sigma = np.exp(rng.normal(-1, 0.3, size=(S, n - 1))).astype(np.float32)
    alpha = rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32)
    for s in range(S):
        t = trees[0 if shared else s]
        lg = centre_logits(t, kinds[s], rng) if n > 3 else rng.normal(0.0, 1.0, n - 1)
        y0 = 1.0 / (1.0 + np.exp(-lg))
        logq0 = t.push_down(np.log(y0), np.log1p(-y0))  # (log of the product of the edge factors)
        xs = logq0 - np.log(eff[s].astype(F64))
        x[s] = (xs - xs.max()).astype(np.float32)
        q, _, _, _ = leaf_masses(x[s], eff[s], True)
        ul, ur = t.sums(q)
        y = ul / (ul + ur)
        mu[s] = (np.log(y) - np.log1p(-y) + sigma[s].astype(F64) * rng.normal(0, 1, n - 1)).astype(np.float32)
    idx = [t.index_arrays() for t in trees]
    L_, R_, F_ = (np.stack([i[j] for i in idx]) for j in range(3))
    out = dict(name=name, n=n, S=S, shared=shared, kinds=kinds, trees=tuple(trees), serial=tuple(serial), x=x, efflen=eff, la_mu=mu,
               la_sigma=sigma, la_alpha=alpha, left_index=L_, right_index=R_, leaf_index=F_)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def tree_of(inp, s):
    return inp["trees"][0 if inp["shared"] else s]


@functools.lru_cache(maxsize=None)
def reference(name, f32_steps=True):
    """density() of every sample of the case, computed once (arrays read-only)"""
    inp = inputs(name)
    out = []
    for s in range(inp["S"]):
        r = density(tree_of(inp, s), inp["x"][s], inp["efflen"][s], inp["la_mu"][s], inp["la_sigma"][s], inp["la_alpha"][s], f32_steps)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return tuple(out)


def mutant(name, s, which):
    inp = inputs(name)
    kw = {"a": dict(sums=sums_from_plain_prefix), "b": dict(tour_prefix=True), "c": dict(sums=sums_one_offset_lost)}[which]
    return density(tree_of(inp, s), inp["x"][s], inp["efflen"][s], inp["la_mu"][s], inp["la_sigma"][s], inp["la_alpha"][s], True, **kw)


def node_gap(got, ref):
    """the largest error of the two tour terms of any node, in units of node_scale (nan counts as infinite)"""
    sc = node_scale(ref)
    with np.errstate(all="ignore"):
        e = np.maximum(np.abs(got["tp0"] - ref["tp0"]), np.abs(got["tp1"] - ref["tp1"])) / sc
    return float(np.where(np.isfinite(e), e, np.inf).max())


def bp_gap(got, ref):
    """the largest error of bp of any leaf, in units of path_abs"""
    with np.errstate(all="ignore"):
        e = np.abs(got["bp"] - ref["bp"]) / ref["path_abs"]
    return float(np.where(np.isfinite(e), e, np.inf).max())


def measure_gaps():
    """(G_node, G_grad, per case figures): the largest scaled gaps between the f32_steps=True and =False results over CASES"""
    per = {}
    for name in CASES:
        n = CASES[name][0]
        gn = gb = gg = lpu = 0.0
        for r32, r64 in zip(reference(name, True), reference(name, False)):
            gn = max(gn, node_gap(r32, r64))
            gb = max(gb, bp_gap(r32, r64))
            gg = max(gg, float((np.abs(r32["x_grad"] - r64["x_grad"]) / grad_scale(r64, n)).max()))
            lpu = max(lpu, abs(r32["lp"] - r64["lp"]) / float(ulp32(r64["lp"])))
        per[name] = dict(node=gn, bp=gb, grad=gg, lp_ulps=lpu)
    return (max(max(v["node"], v["bp"]) for v in per.values()), max(v["grad"] for v in per.values()), per)


# The largest scaled gap between the Float32-step and the all-Float64 restatement over all of CASES: of the nodes' tour terms in units
# of (1 + |y_grad|) / u and of bp in units of path_abs (G_NODE, the larger of the two), and of x_grad in units of grad_scale
# (G_GRAD).  The device may differ from the Float32-step restatement by roundings of the same class and number -- its expf, logf,
# sinhf, coshf and log1pf may each be a few ulp from NumPy's, and it forms z through z_std cosh(alpha) - sqrt(1 + z_std^2)
# sinh(alpha) -- so it is allowed 8 G; nothing here is fitted to the device.  Produced by
#     python tests/approx_density_restatement.py
# (tests/test_approx_density_host.py recomputes them and asserts that they still are what is written here).  G_NODE is a maximum over
# 27 000 nodes and sits where y_grad = (d_logit + 2 y - 1) / (y (1 - y)) cancels, so that the unit (1 + |y_grad|) / u is small
# against the rounding noise of d_logit / (y (1 - y)): 6.6e-4 on one node of the 3 000-leaf caterpillar, 1e-5 typically.
G_NODE = 6.644e-04
G_GRAD = 1.653e-05
T_NODE = 8 * G_NODE
T_GRAD = 8 * G_GRAD

# The node SUMS have a sharper, derived bound.  The combination y tp1 + (1 - y) tp0 of a node's two tour terms is -1/u whatever
# y_grad is, so with the restatement's y it shows the implementation's u free of the noise of y_grad.  What may differ is every q:
# by an ulp of the Float32 exp(x) (2^-23 relative) and by the roundings to Float32 on the way to q -- one in an implementation that
# rounds exp(x) efflen / sum once, three here (p, p * efflen, q), at 2^-24 each -- so by 3 * 2^-23 in all, and every sum of q with
# it: at most 2^-21 / u on 1/u.  y = u_left / u then differs by 2^-20 y (1 - y) at most, which the combination multiplies by
# tp1 - tp0 = y_grad / u.  With E_U = 2^-20:
#     |y tp1 + (1 - y) tp0 + 1/u| <= E_U (1 + y (1 - y) |y_grad|) / u
E_U = 2.0 ** -20


def sum_gap(got, ref):
    """the largest error of -(y tp1 + (1 - y) tp0) = 1/u of any node, in units of (1 + y (1 - y) |y_grad|) / u (nan: infinite)"""
    y, u = ref["y"], ref["u"]
    with np.errstate(all="ignore"):
        e = np.abs(y * got["tp1"] + (1.0 - y) * got["tp0"] + 1.0 / u) * u / (1.0 + y * (1.0 - y) * np.abs(ref["y_grad"]))
    return float(np.where(np.isfinite(e), e, np.inf).max())


def input_conditions(name):
    """What the inputs must satisfy for the checks to mean something, from the restatement alone; returns the case's figures."""
    inp, n = inputs(name), CASES[name][0]
    fig = []
    for s, r in enumerate(reference(name, True)):
        q32 = r["q"].astype(np.float32)
        assert (q32 >= np.finfo(np.float32).tiny).all(), (name, s, "a q is 0 or subnormal as Float32")
        ymin = float(np.minimum(r["y"], 1.0 - r["y"]).min())
        assert ymin >= 1e-9, (name, s, ymin)
        umin, kind = float(r["u"].min()), inp["kinds"][s]
        if n >= 513:
            bound = 1e-15 if (n >= 1024 and not _is_spine(kind)) else (1e-9 if (n == 3000 and _is_spine(kind)) else 1e-11)
            assert umin <= bound, (name, s, kind, umin, bound)
        fig.append(dict(umin=umin, ymin=ymin, decades=float(np.log10(r["q"].max() / r["q"].min())), zmax=float(np.abs(r["z"]).max())))
    return fig


if __name__ == "__main__":
    g_node, g_grad, per = measure_gaps()
    for name, v in per.items():
        print("%-14s node %.3e  bp %.3e  grad %.3e  |lp32 - lp64| %.3f ulp" % (name, v["node"], v["bp"], v["grad"], v["lp_ulps"]))
    print("G_NODE = %.3e\nG_GRAD = %.3e" % (g_node, g_grad))

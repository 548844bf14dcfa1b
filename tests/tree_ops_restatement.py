"""Plain NumPy restatement of the reference's tree recursions -- transform!, transform_gradients!, inverse_transform!
(src/ptt.jl:125-285) and the TensorFlow ops HSB, InvHSB, InvHSBGrad (hsb_ops.cpp:87-109, 212-238, 342-391) -- written as the
reference's walks: top-down products, bottom-up subtree sums, the g1/g2 recursion.  No prefix differences, which is the device's
own algorithm (polee_amd/csrc/scan.hpp).  Every function runs in float64 or, with dtype=np.longdouble, in the host's long double;
the gap between the two is what the float64 values are trusted to.  A helper module, not a test file.  It also holds the input
builders of tests/test_gpu_tree_saturation.py and tests/test_gpu_tree_ops_large.py, the constant C_PATH and three CPU-only mutants
of the device's scan (tests/test_tree_ops_host.py).

Saturated nodes.  A stick fraction y of exactly 1 gives the right child u = 0 (y = 0: the left child), and so every node and leaf
below it: the reference's products simply carry the 0 down.  Leaves with u = 0 come out at transform!'s floor of 1e-16 (0 for the
HSB op, which has no floor), and ladj = sum log u is -inf as soon as a dead child is an internal node.
"""
import functools

import numpy as np

F64, LD = np.float64, np.longdouble
CHUNK = 512  # entries per chunk of the device's scans (SCAN_CHUNK); the restatement itself has no chunks
SPINE_THREADS = 256  # threads of the device's spine kernel, each with ceil(nchunks / 256) chunk totals
FLOOR = 1e-16


# ---- trees ------------------------------------------------------------------------------------------------------------------

def build_tree(n, rng, kind):
    """Serialised tree (node_parent_idxs, node_js) as the reference writes it (DFS pre-order, the RIGHT child first), in O(n).
    kind: 'random' (every subtree split at a uniform quarter-to-three-quarters point), 'balanced', 'spine' (a caterpillar whose
    single leaves hang on a random side)."""
    perm = rng.permutation(n) + 1
    coin = rng.random(max(n - 1, 1))
    parents, js = [], []
    stack = [(n, 0)]
    nleaf = nint = 0
    while stack:
        size, par = stack.pop()
        idx = len(parents) + 1
        parents.append(par)
        if size == 1:
            js.append(int(perm[nleaf]))
            nleaf += 1
            continue
        js.append(0)
        c = coin[nint]
        nint += 1
        if kind == "spine":
            a = 1 if c < 0.5 else size - 1
        elif kind == "balanced":
            a = size // 2
        else:
            a = min(max(int(size * (0.25 + 0.5 * c)), 1), size - 1)
        stack.append((size - a, idx))  # left: pushed first ...
        stack.append((a, idx))         # ... so that the right child is popped, and listed, first
    return np.array(parents, np.int32), np.array(js, np.int32)


class Tree:
    """Child arrays of a serialised tree; the internal nodes are numbered k = 0.. in array order (ptt.jl:132-154)."""

    def __init__(self, parents, js):
        parents, js = np.asarray(parents, np.int64), np.asarray(js, np.int64)
        N = len(parents)
        self.parents, self.js = parents.astype(np.int32), js.astype(np.int32)
        self.N, self.n = N, (N + 1) // 2
        left, right = [-1] * N, [-1] * N
        for i, p in enumerate((parents - 1).tolist()):
            if i == 0:
                continue
            assert 0 <= p < i
            if right[p] < 0:
                right[p] = i
            else:
                assert left[p] < 0
                left[p] = i
        self.left, self.right = np.array(left, np.int64), np.array(right, np.int64)
        self.leaf = js - 1  # 0-based transcript, -1 for internal nodes
        self.nodes = np.flatnonzero(self.leaf < 0)  # k -> node
        self.leaves = np.flatnonzero(self.leaf >= 0)
        assert len(self.nodes) == self.n - 1
        self._l, self._r = left, right
        self._internal = (self.leaf < 0).tolist()
        size = [1] * N
        for i in range(N - 1, -1, -1):
            if self._internal[i]:
                size[i] = size[left[i]] + size[right[i]]
        self.size = np.array(size, np.int64)

    def index_arrays(self):
        """left_index, right_index, leaf_index as the TF ops take them (0-based, -1 = none)"""
        return self.left.astype(np.int32), self.right.astype(np.int32), self.leaf.astype(np.int32)

    def by_transcript(self, per_node):
        out = np.empty(self.n, per_node.dtype)
        out[self.leaf[self.leaves]] = per_node[self.leaves]
        return out


def stick_ys(tree, rng, B):
    """Stick fractions that keep every leaf of a deep tree above the floor: a node with s leaves below it gives its smaller
    side U(0.5, 1.5) / s of them per leaf (tests/test_gpu_fullsize.py draws a spine's the same way)."""
    k = tree.nodes
    s, sl = tree.size[k].astype(F64), tree.size[tree.left[k]].astype(F64)
    y = sl / s * rng.uniform(0.5, 1.5, size=(B, len(k)))
    big_left = sl > s / 2
    y = np.where(big_left, 1.0 - (s - sl) / s * rng.uniform(0.5, 1.5, size=(B, len(k))), y)
    return np.clip(y, 1e-6, 1 - 1e-6)


def _scalars(a, dtype):
    """a vector as a list of scalars: Python floats for float64 (the same IEEE arithmetic, several times faster in a loop)"""
    a = np.asarray(a, dtype)
    return a.tolist() if dtype is F64 else list(a)


# ---- the reference's walks ------------------------------------------------------------------------------------------------------

def node_values(tree, ys, dtype=F64):
    """u of every node, top-down (ptt.jl:131-148): u_root = 1, u_left = y u, u_right = (1 - y) u."""
    y = _scalars(ys, dtype)
    one = dtype(1) if dtype is not F64 else 1.0
    u = [one] * tree.N
    l, r, internal = tree._l, tree._r, tree._internal
    k = 0
    for i in range(tree.N):
        if internal[i]:
            ui, yk = u[i], y[k]
            u[l[i]] = yk * ui
            u[r[i]] = (one - yk) * ui
            k += 1
    return np.array(u, dtype)


def _log(u):
    with np.errstate(divide="ignore"):
        return np.log(u)


def transform(tree, ys, dtype=F64, floor=FLOOR):
    """transform! -> (xs f32 with the leaf floor, ladj, u per node).  floor = 0: the HSB op."""
    u = node_values(tree, ys, dtype)
    ul = tree.by_transcript(u)
    xs = np.maximum(ul.astype(np.float32).astype(F64), floor).astype(np.float32)
    ladj = _log(u[tree.nodes]).sum() if tree.n > 1 else dtype(0)
    return xs, ladj, u


def logistic_y(logit):
    """hsb_ops.cpp:103: exp of the float, the rest in double"""
    logit = np.asarray(logit, np.float32)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-logit).astype(F64))


def hsb(tree, logit):
    return transform(tree, logistic_y(logit), floor=0.0)[0]


def sampler_logits(mu, sigma, alpha, z0):
    """z = sinh(asinh z0 + alpha), y_logit = mu + sigma z, in Float32"""
    mu, sigma, alpha, z0 = (np.asarray(a, np.float32) for a in (mu, sigma, alpha, z0))
    zs = np.sinh(np.arcsinh(z0) + alpha).astype(np.float32)
    return (mu + zs * sigma).astype(np.float32)


def sampler_ys(mu, sigma, alpha, z0, y_eps=0.0):
    """rand! (approx-sampler.jl:37-44): y = logistic(mu + sigma z) in Float32, exactly 1 from a logit of 16.64 on; y_eps > 0 is
    the clamp of the initial-value draws (estimate.jl:443-447)."""
    with np.errstate(over="ignore"):
        y = (np.float32(1) / (np.float32(1) + np.exp(-sampler_logits(mu, sigma, alpha, z0)))).astype(F64)
    return np.clip(y, y_eps, 1 - y_eps) if y_eps > 0 else y


def sampler_draw(tree, mu, sigma, alpha, z0):
    return transform(tree, sampler_ys(mu, sigma, alpha, z0))[0]


def x0_draw(tree, mu, sigma, alpha, efflens, z0):
    """one draw of the initial values (estimate.jl:436-455): clamped y, divided by the effective lengths, renormalised"""
    x = transform(tree, sampler_ys(mu, sigma, alpha, z0, 1e-10))[0] / np.asarray(efflens, np.float32)
    return x / np.float32(np.cumsum(x, dtype=np.float32)[-1])


def tf_sampler(tree, mu, sigma, alpha, efflens, z0):
    """rnaseq_approx_likelihood_sampler (polee_approx_likelihood.py:35-59) for one sample: the HSB op's logistic, whose double
    is exactly 1 only from a logit of 36.8 on"""
    x = hsb(tree, sampler_logits(mu, sigma, alpha, z0)) / np.asarray(efflens, np.float32)
    x = (x.astype(F64) / x.astype(F64).sum()).astype(np.float32)
    return np.clip(x, np.float32(1e-16), np.float32(0.99999999))


def subtree_sums(tree, x, dtype=F64):
    """u of every node, bottom-up (ptt.jl:265-276): the leaves' x, summed"""
    u = [None] * tree.N
    xs = _scalars(np.asarray(x).astype(dtype), dtype)
    l, r, internal, leaf = tree._l, tree._r, tree._internal, tree.leaf.tolist()
    for i in range(tree.N - 1, -1, -1):
        u[i] = u[l[i]] + u[r[i]] if internal[i] else xs[leaf[i]]
    return np.array(u, dtype)


def inverse(tree, x, dtype=F64):
    """inverse_transform! / InvHSB -> (ys, ladj with the log of Float32(u) as ptt.jl:277 takes it, ladj with the double's log as
    hsb_ops.cpp:230 does, u per node)"""
    u = subtree_sums(tree, x, dtype)
    k = tree.nodes
    ys = u[tree.left[k]] / u[k]
    ladj_jl = -np.log(u[k].astype(np.float32)).astype(dtype).sum()
    ladj_tf = -np.log(u[k]).sum()
    return ys, ladj_jl, ladj_tf, u


def y_gradients(tree, ys, u, x_grad, with_ladj=True, dtype=F64):
    """transform_gradients! (ptt.jl:167-209; with_ladj=False: :217-251) with no Float32 intermediates -> (y_grad, term): term is
    the sum of the magnitudes of the two terms whose difference y_grad is."""
    y, uu, xg = _scalars(ys, dtype), _scalars(u, dtype), _scalars(x_grad, dtype)
    zero = dtype(0) if dtype is not F64 else 0.0
    one = dtype(1) if dtype is not F64 else 1.0
    N = tree.N
    g1, g2 = [zero] * N, [zero] * N
    out, term = [zero] * (tree.n - 1), [zero] * (tree.n - 1)
    l, r, internal, leaf = tree._l, tree._r, tree._internal, tree.leaf.tolist()
    k = tree.n - 2
    for i in range(N - 1, -1, -1):
        if not internal[i]:
            g1[i] = xg[leaf[i]]
            continue
        a, b = g1[l[i]] + g2[l[i]], g1[r[i]] + g2[r[i]]
        out[k] = uu[i] * (a - b)
        term[k] = uu[i] * (abs(a) + abs(b))
        g1[i] = y[k] * g1[l[i]] + (one - y[k]) * g1[r[i]]
        if with_ladj:
            g2[i] = one / uu[i] + y[k] * g2[l[i]] + (one - y[k]) * g2[r[i]]
        k -= 1
    return np.array(out, dtype), np.array(term, dtype)


def inv_hsb_grad(tree, y_grad, ladj_grad, y, dtype=F64):
    """InvHSBGrad (hsb_ops.cpp:342-391): v_child = v - ladj_grad / u +- (u_other / u^2) y_grad down the tree with u recomputed from
    y -> (backprops by transcript, path_abs: the sum of the magnitudes of the edge terms on the leaf's path, log u per node)."""
    yy, yg = _scalars(y, dtype), _scalars(y_grad, dtype)
    lg = dtype(np.float32(ladj_grad)) if dtype is not F64 else float(np.float32(ladj_grad))
    zero = dtype(0) if dtype is not F64 else 0.0
    one = dtype(1) if dtype is not F64 else 1.0
    N = tree.N
    u, v, pa = [one] * N, [zero] * N, [zero] * N
    l, r, internal = tree._l, tree._r, tree._internal
    k = 0
    for j in range(N):
        if not internal[j]:
            continue
        uj, yk = u[j], yy[k]
        ul, ur = uj * yk, uj * (one - yk)
        d = -one / uj * lg
        uj2 = uj * uj
        tl, tr = d + (ur / uj2) * yg[k], d - (ul / uj2) * yg[k]
        v[l[j]], v[r[j]] = v[j] + tl, v[j] + tr
        pa[l[j]], pa[r[j]] = pa[j] + abs(tl), pa[j] + abs(tr)
        u[l[j]], u[r[j]] = ul, ur
        k += 1
    ua = np.array(u, dtype)
    return tree.by_transcript(np.array(v, dtype)), tree.by_transcript(np.array(pa, dtype)), _log(ua)


# ---- the library's plan and the placements of saturated nodes --------------------------------------------------------------------

def ptt_plan(parents, js):
    """polee_debug_ptt_plan: the Euler tour the device scans (host code of the library; no GPU needed).  Adds, per internal node
    k and side (0 right, 1 left), the tour positions of the child's ENTER and EXIT (-1: the child is a leaf)."""
    import ctypes as C
    from polee_amd import _lib as L
    pp, jj = np.ascontiguousarray(parents, np.int32), np.ascontiguousarray(js, np.int32)
    N = len(pp)
    n = (N + 1) // 2
    TL = 3 * n - 2
    code, tgt, ltid = np.zeros(TL, np.uint32), np.zeros(TL, np.int32), np.zeros(n, np.int32)
    lo, mid, hi1 = (np.zeros(max(n - 1, 1), np.int32) for _ in range(3))
    depth = C.c_int32()
    L.check(L.lib().polee_debug_ptt_plan(L.ptr(pp, L.i32p), L.ptr(jj, L.i32p), N, L.ptr(code, L.u32p), L.ptr(tgt, L.i32p),
                                         L.ptr(ltid, L.i32p), L.ptr(lo, L.i32p), L.ptr(mid, L.i32p), L.ptr(hi1, L.i32p),
                                         C.byref(depth)))
    typ, root, side, kpar = code & 3, (code & 4) != 0, ((code >> 3) & 1).astype(np.int64), (code >> 4).astype(np.int64)
    enter, exit_ = np.full((max(n - 1, 1), 2), -1, np.int64), np.full((max(n - 1, 1), 2), -1, np.int64)
    e = np.flatnonzero((typ == 0) & ~root)
    enter[kpar[e], side[e]] = e
    e = np.flatnonzero((typ == 1) & ~root)
    exit_[kpar[e], side[e]] = e
    return dict(n=n, TL=TL, code=code, tgt=tgt, leaf_tid=ltid, lo=lo[:n - 1], mid=mid[:n - 1], hi1=hi1[:n - 1], enter=enter,
                exit=exit_, typ=typ)


# y that kills the child on `side` (0 right, 1 left): u_right = (1 - y) u, u_left = y u
DEAD_Y = {0: 1.0, 1: 0.0}
PLACEMENTS = ("one_y1", "one_y0", "root", "leaf_child", "internal_same_chunk", "internal_cross_chunk", "nested", "random5")


def placement(pl, name, rng):
    """{k: y} for one placement of saturated nodes, chosen from the plan; None where the tree has no such node."""
    n, enter, exit_ = pl["n"], pl["enter"], pl["exit"]
    internal = enter >= 0
    if name == "one_y1":
        return {(n - 1) // 2: 1.0}
    if name == "one_y0":
        return {(n - 1) // 3: 0.0}
    if name == "root":
        return {0: 1.0}
    if name == "leaf_child":
        ks, sides = np.nonzero(~internal)
        i = len(ks) // 2
        return {int(ks[i]): DEAD_Y[int(sides[i])]}
    same = internal & (enter // CHUNK == exit_ // CHUNK)
    last = (pl["TL"] - 1) // CHUNK
    cross = internal & (enter // CHUNK != exit_ // CHUNK) & (exit_ // CHUNK == last) & (pl["TL"] % CHUNK != 0)
    if name in ("internal_same_chunk", "internal_cross_chunk"):
        ks, sides = np.nonzero(same if name == "internal_same_chunk" else cross)
        if len(ks) == 0:
            return None
        # the middle one within a chunk; across chunks the one whose EXIT comes first, so that live leaves follow it in the
        # last chunk (behind the last EXITs of a tour there are none, and nothing would show a poisoned prefix)
        i = len(ks) // 2 if name == "internal_same_chunk" else int(np.argmin(exit_[ks, sides]))
        return {int(ks[i]): DEAD_Y[int(sides[i])]}
    if name == "nested":
        span = np.where(internal, exit_ - enter, 0)
        ks, sides = np.nonzero(span >= 4)  # the dead child has an internal child of its own
        if len(ks) == 0:
            return None
        i = len(ks) // 2
        k, s = int(ks[i]), int(sides[i])
        inside = np.flatnonzero((pl["typ"][enter[k, s] + 1:exit_[k, s]] == 0)) + enter[k, s] + 1
        k2 = int(pl["tgt"][inside[len(inside) // 2]])
        kc = int(pl["tgt"][enter[k, s]])  # the dead child itself, saturated as well
        return {k: DEAD_Y[s], kc: 1.0, k2: 0.0}
    if name == "random5":
        m = max((n - 1) // 20, 1)
        ks = rng.choice(n - 1, size=m, replace=False)
        return {int(k): float(v) for k, v in zip(ks, rng.integers(0, 2, size=m))}
    raise KeyError(name)


SAT_TREES = (("fixture", 313), ("random", 1100), ("spine", 1100), ("balanced", 1024), ("random", 2), ("random", 3))


@functools.lru_cache(maxsize=None)
def sat_tree(kind, n):
    """(Tree, plan) of a part-A tree; the fixture's is the golden prepared sample's"""
    if kind == "fixture":
        import os
        a = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mBr_M_6w_1.prep.npz"))
        p, js = a["node_parent_idxs"], a["node_js"]
    else:
        # (a seed whose random tree of 1100 leaves has an internal child that closes in the last chunk with leaves behind it:
        # tests/test_tree_ops_host.py asserts that)
        p, js = build_tree(n, np.random.default_rng(7001 + n), kind)
    t = Tree(p, js)
    assert t.n == n
    return t, ptt_plan(t.parents, t.js)


@functools.lru_cache(maxsize=None)
def sat_cases():
    """[(kind, n, placement name)] for every placement the tree has"""
    out = []
    for kind, n in SAT_TREES:
        _, pl = sat_tree(kind, n)
        for name in PLACEMENTS:
            if placement(pl, name, np.random.default_rng(1)) is not None:
                out.append((kind, n, name))
    return tuple(out)


def sat_inputs(kind, n, name, B=1, seed=0):
    """(tree, plan, {k: y}, clean ys [B][n-1]): the clean stick fractions of a case and where it saturates them"""
    t, pl = sat_tree(kind, n)
    rng = np.random.default_rng([seed, n, PLACEMENTS.index(name)])
    where = placement(pl, name, rng)
    ys = stick_ys(t, rng, B) if kind == "spine" else rng.uniform(0.3, 0.7, size=(B, n - 1))
    return t, pl, where, ys


def saturate(ys, where):
    ys = np.array(ys, F64)
    for k, v in where.items():
        ys[..., k] = v
    return ys


def logits_of(ys):
    with np.errstate(divide="ignore"):
        return (np.log(ys) - np.log1p(-ys)).astype(np.float32)


def saturated_logits(ys, where, big):
    """Float32 logits of the clean ys with +big where y is to be 1 and -big where 0"""
    logit = logits_of(ys)
    for k, v in where.items():
        logit[..., k] = big if v == 1.0 else -big
    return logit


def sampler_params(nm1, where, rng, ones=(17.0, 30.0)):
    """mu, sigma, alpha, z0, efflens of a sampler whose chosen nodes saturate: mu = 17 (logistic_f32 is exactly 1 above 16.64)
    and 30 in turn where y is to be 1, -120 where 0 (-17 and -30 do not reach 0 in Float32), sigma tiny on those nodes.  The
    other nodes' y stay near (0.3, 0.7), also on a spine (whose deep leaves then lie at the floor): a Float32 y next to 1 has
    1 - y to three digits only, and one ulp between two libraries' expf would count as an error of the tree."""
    mu = logits_of(rng.uniform(0.3, 0.7, nm1))
    sigma = np.exp(rng.normal(-2, 0.5, nm1)).astype(np.float32)
    alpha = rng.normal(0, 0.3, nm1).astype(np.float32)
    for i, (k, v) in enumerate(sorted(where.items())):
        mu[k] = ones[i % 2] if v == 1.0 else -120.0
        sigma[k] = 1e-3
    z0 = rng.normal(size=nm1).astype(np.float32)
    eff = rng.uniform(200, 3000, nm1 + 1).astype(np.float32)
    return mu, sigma, alpha, z0, eff


@functools.lru_cache(maxsize=None)
def near_saturated_sampler(kind, n, N=3):
    """(mu, sigma, alpha, z0 [N][n-1], transcripts): a clean sampler with mu = -17 on one node and -30 on another -- almost
    saturated, y = 4e-8 and 9e-14 in Float32, but live.  The two nodes are those with the largest u among the nodes whose left
    child is a leaf, so that the leaf's y u stays above the 1e-16 floor; `transcripts` are those two leaves."""
    t, _ = sat_tree(kind, n)
    rng = np.random.default_rng([n, 17])
    mu, sigma, alpha, _, _ = sampler_params(n - 1, {}, rng)
    z0 = rng.normal(size=(N, n - 1)).astype(np.float32)
    u = node_values(t, sampler_ys(mu, sigma, alpha, z0[0]))
    cand = np.flatnonzero(t.leaf[t.left[t.nodes]] >= 0)
    ks = cand[np.argsort(-u[t.nodes[cand]])[:2]]
    mu[ks] = (-17.0, -30.0)
    sigma[ks] = 1e-3
    return mu, sigma, alpha, z0, t.leaf[t.left[t.nodes[ks]]]


def ladj_matches(got, ref):
    """never NaN; -inf exactly where the reference's is; else within 1e-10 max(1, |ladj|)"""
    if np.isnan(got):
        return False
    if np.isinf(ref):
        return got == ref
    return abs(got - ref) <= 1e-10 * max(1.0, abs(ref))


# ---- part B: sizes where the device's spine changes regime ------------------------------------------------------------------------

LARGE_CASES = (("random", 342), ("random", 43691), ("random", 43692), ("random", 43862), ("random", 131072), ("random", 131073),
               ("balanced", 43692), ("spine", 43692), ("balanced", 131073), ("spine", 131073))

# inv_hsb_grad is allowed one f32 ulp of the reference plus C_PATH * path_abs: ten times the largest gap between the float64 and
# the long double run of inv_hsb_grad over LARGE_CASES, in units of path_abs (the device's scan adds the same terms in another
# order).  Printed by
#     python -c "import sys; sys.path.insert(0, 'tests'); import tree_ops_restatement as R; print(R.measure_c_path())"
# which gave 2.06e-13 on x86-64 (80-bit long double); tests/test_tree_ops_host.py recomputes it.
C_PATH_MEASURED = 2.1e-13
C_PATH = 10 * C_PATH_MEASURED


@functools.lru_cache(maxsize=None)
def large_tree(kind, n):
    return Tree(*build_tree(n, np.random.default_rng(9000 + n), kind))


@functools.lru_cache(maxsize=None)
def large_inputs(kind, n):
    """ys, x_grad, x (a Dirichlet(0.5) draw floored at 1e-12, f32), logits, y_grad and ladj_grad of the InvHSB gradient; B = 2 rows"""
    t = large_tree(kind, n)
    rng = np.random.default_rng([n, len(kind)])
    B = 2
    ys = stick_ys(t, rng, B) if kind == "spine" else rng.uniform(0.3, 0.7, size=(B, n - 1))
    x = rng.gamma(0.5, size=(B, n))
    x = np.maximum((x / x.sum(axis=1, keepdims=True)).astype(np.float32), np.float32(1e-12))
    with np.errstate(divide="ignore"):
        logit = (np.log(ys) - np.log1p(-ys)).astype(np.float32)
    d = dict(ys=ys, x_grad=rng.normal(size=(B, n)) * 10, x=x, logit=logit, y_grad=rng.normal(size=(B, n - 1)),
             ladj_grad=rng.normal(size=B).astype(np.float32))
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def large_reference(kind, n, dtype=F64):
    """every reference quantity of a part-B case, rows stacked; computed once and shared"""
    t, d = large_tree(kind, n), large_inputs(kind, n)
    out = {k: [] for k in ("xs", "u_leaf", "ladj", "yg", "yg_term", "yg0", "yg0_term", "inv_y", "inv_ladj_jl", "inv_ladj_tf", "hsb",
                           "hsb_u", "bp", "path_abs", "logu")}
    for b in range(2):
        xs, ladj, u = transform(t, d["ys"][b], dtype)
        out["xs"].append(xs); out["ladj"].append(ladj); out["u_leaf"].append(t.by_transcript(u))
        g, term = y_gradients(t, d["ys"][b], u, d["x_grad"][b], True, dtype)
        out["yg"].append(g); out["yg_term"].append(term)
        g, term = y_gradients(t, d["ys"][b], u, d["x_grad"][b], False, dtype)
        out["yg0"].append(g); out["yg0_term"].append(term)
        iy, ljl, ltf, _ = inverse(t, d["x"][b], dtype)
        out["inv_y"].append(iy); out["inv_ladj_jl"].append(ljl); out["inv_ladj_tf"].append(ltf)
        hx, _, hu = transform(t, logistic_y(d["logit"][b]), dtype, floor=0.0)
        out["hsb"].append(hx); out["hsb_u"].append(t.by_transcript(hu))
        # (the gradient's y input is the float64 run's, whichever precision this run has: the same input for both)
        y_in = np.asarray(iy, F64) if dtype is F64 else large_reference(kind, n, F64)["inv_y"][b]
        bp, pa, logu = inv_hsb_grad(t, d["y_grad"][b], d["ladj_grad"][b], y_in, dtype)
        out["bp"].append(bp); out["path_abs"].append(pa); out["logu"].append(logu)
    out = {k: np.stack(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def f32_ulp(x):
    x = np.abs(np.asarray(x, F64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(F64)


def measure_c_path(cases=LARGE_CASES):
    worst = 0.0
    for kind, n in cases:
        a, b = large_reference(kind, n, F64), large_reference(kind, n, LD)
        worst = max(worst, float(np.max(np.abs(a["bp"] - b["bp"]) / b["path_abs"])))
    return worst


# the bounds of part B as scaled errors: a value <= 1 passes
def scaled_errors(kind, n, got, ref=None):
    """{operation: worst |got - ref| / bound} for the outputs in `got` (same keys as large_reference)"""
    r = large_reference(kind, n) if ref is None else ref
    out = {}

    def rel(key, rtol, refkey=None):
        a, b = np.asarray(got[key], F64), np.asarray(r[refkey or key], F64)
        out[key] = float(np.max(np.abs(a - b) / (rtol * np.abs(b))))
    if "xs" in got:
        rel("xs", 3e-7)
    if "ladj" in got:
        out["ladj"] = float(np.max(np.abs(got["ladj"] - r["ladj"]) / (1e-10 * np.maximum(1, np.abs(r["ladj"])))))
    for key in ("yg", "yg0"):
        if key in got:
            out[key] = float(np.max(np.abs(got[key] - r[key]) / (1e-9 * (r[key + "_term"] + 1))))
    if "inv_y" in got:
        rel("inv_y", 1e-12)
    for key in ("inv_ladj_jl", "inv_ladj_tf"):
        if key in got:
            out[key] = float(np.max(np.abs(got[key] - r[key]) / (1e-5 * np.maximum(1, np.abs(r[key])))))
    if "hsb" in got:
        rel("hsb", 1e-6)
    if "bp" in got:
        out["bp"] = float(np.max(np.abs(got["bp"] - r["bp"]) / (f32_ulp(r["bp"]) + C_PATH * r["path_abs"])))
    return out


# ---- CPU-only mutants of the device's scan --------------------------------------------------------------------------------------

def _chunk_offsets(totals, mutant):
    """exclusive scan of the chunk totals as scan_spine_kernel makes it: thread t owns chunks [t per, (t+1) per)"""
    nch = len(totals)
    per = -(-nch // SPINE_THREADS)
    off = np.zeros(nch, totals.dtype)
    acc = totals[0] * 0
    for b in range(0, nch, per):
        e = min(b + per, nch)
        run = acc
        for i in range(b, e):
            off[i] = run
            if not (mutant == "spine_first_total" and i == b and e - b > 1):
                run = run + totals[i]
        acc = acc + totals[b:e].sum()
    return off


def chunked_prefix(values, mutant=None):
    """inclusive prefix of `values` as the device's three-phase scan builds it (chunks of CHUNK, spine, apply) -- in float64 for
    float64 values (the tour scan), exactly for an object array of Python ints (the double-double leaf scan, 1e-32 relative) --
    and with one of the faults the part-B sizes exist to catch:
      'spine_first_total'  a spine thread leaves its first chunk's total out of the offsets of its later chunks
      'partial_tail'       the last element of a partial last chunk is dropped (taken as 0)"""
    v = np.array(values)
    if mutant == "partial_tail" and len(v) % CHUNK:
        v[-1] = v[-1] * 0
    nch = -(-len(v) // CHUNK)
    pad = np.zeros(nch * CHUNK, v.dtype)
    pad[:len(v)] = v
    pad = pad.reshape(nch, CHUNK)
    inc = np.cumsum(pad, axis=1)
    off = _chunk_offsets(inc[:, -1].copy(), mutant)
    return (inc + off[:, None]).reshape(-1)[:len(v)]


LEAF_SCALE = 2.0 ** 64  # an f32 x >= 1e-12 is a whole multiple of 2^-64


def leaf_prefix(xl, mutant=None):
    """exclusive prefix C[0..n] over leaf order as the device's double-double scan holds it; mutant 'no_low_word': each prefix
    rounded to one double, as a scan that dropped the low words would leave it"""
    ints = np.array([int(v) for v in (np.asarray(xl, F64) * LEAF_SCALE).tolist()], object)
    C = np.concatenate([np.array([0], object), chunked_prefix(ints, mutant)])
    if mutant == "no_low_word":
        C = np.array([float(c) for c in C], object)
    return C


def _diff(C, hi, lo):
    return np.array([float(a - b) for a, b in zip(C[hi], C[lo])], F64) / LEAF_SCALE


def emulate_device(kind, n, mutant=None):
    """The part-B outputs as the device's algorithm computes them (tour prefix of signed edge logs; leaf-order prefix and its
    differences), from the plan, in float64 -- the subject of the mutants."""
    t, d = large_tree(kind, n), large_inputs(kind, n)
    pl = ptt_plan(t.parents, t.js)
    code, typ, tgt = pl["code"], pl["typ"], pl["tgt"]
    rootf, side, kpar = (code & 4) != 0, (code & 8) != 0, np.minimum(code >> 4, max(n - 2, 0)).astype(np.int64)
    leaf = typ == 2
    got = {k: [] for k in ("xs", "ladj", "inv_y", "inv_ladj_tf")}
    for b in range(2):
        ys = d["ys"][b]
        lf = np.where(rootf, 0.0, np.where(side, np.log(ys[kpar]), np.log1p(-ys[kpar])))
        val = np.where(typ == 0, lf, np.where(typ == 1, -lf, 0.0))
        incl = chunked_prefix(val, None if mutant == "no_low_word" else mutant)
        ul = np.zeros(n)
        ul[tgt[leaf]] = np.exp(incl[leaf] + lf[leaf])
        x = np.zeros(n)
        x[pl["leaf_tid"]] = ul
        got["xs"].append(np.maximum(x.astype(np.float32).astype(F64), FLOOR).astype(np.float32))
        got["ladj"].append(incl[typ == 0].sum())
        xl = d["x"][b].astype(F64)[pl["leaf_tid"]]
        C = leaf_prefix(xl, mutant)
        ur, ul_ = _diff(C, pl["mid"], pl["lo"]), _diff(C, pl["hi1"], pl["mid"])
        with np.errstate(all="ignore"):  # (a mutant's subtree sums may be 0 or negative)
            got["inv_y"].append(ul_ / (ul_ + ur))
            got["inv_ladj_tf"].append(-np.log(ul_ + ur).sum())
    return {k: np.stack(v) for k, v in got.items()}

"""The density of the fitted approximation and its gradient (polee_amd/csrc/approx.hip) node by node against the float64 restatement
(tests/approx_density_restatement.py, its Float32-step mode), on trees of more than one chunk of 512 leaves: n just below, at and
above the chunk size, balanced trees whose nodes end exactly on chunk multiples, caterpillars (nearly every node crosses chunks; more
than one block of crossing nodes), caterpillars whose nodes all start in chunk 0 or all end at n, one handle holding trees of three
shapes, and the library's two fallback paths (POLEE_APPROX_NO_CHUNKS, POLEE_APPROX_NO_OPEN_LISTS).  The inputs span 15 to 22 decades of
q with z = O(1), so a double-double prefix that lost its low word, or a chunk offset that is not added, moves the node terms far
beyond the tolerances -- which the public outputs (lp as Float32, x_grad = q * ...) would not show.  The per-node observables come
through the read-only hook polee_debug_approx_node_terms.  Tolerances: T.T_NODE, T.T_GRAD, T.E_U, none of them fitted to the device
(tests/test_approx_density_host.py)."""
import ctypes as C

import numpy as np
import pytest

import approx_density_restatement as T

pytestmark = pytest.mark.gpu

VARIANTS = {"default": (), "no_chunks": ("POLEE_APPROX_NO_CHUNKS",), "no_open_lists": ("POLEE_APPROX_NO_OPEN_LISTS",),
            "neither": ("POLEE_APPROX_NO_CHUNKS", "POLEE_APPROX_NO_OPEN_LISTS")}
RUNS = [(name, "default") for name in T.CASES] + [(name, v) for name in T.VARIANT_CASES for v in VARIANTS if v != "default"]


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


def _plan(parents, js):
    """the library's own order of nodes and leaves (polee_debug_ptt_plan): lo, mid, hi1 per node k, leaf_tid per leaf position"""
    from polee_amd import _lib as L
    N = len(parents)
    n = (N + 1) // 2
    code, tgt, ltid = np.zeros(3 * n - 2, np.uint32), np.zeros(3 * n - 2, np.int32), np.zeros(n, np.int32)
    lo, mid, hi1 = (np.zeros(n - 1, np.int32) for _ in range(3))
    depth = C.c_int32()
    pp, jj = np.ascontiguousarray(parents, np.int32), np.ascontiguousarray(js, np.int32)
    L.check(L.lib().polee_debug_ptt_plan(L.ptr(pp, L.i32p), L.ptr(jj, L.i32p), N, L.ptr(code, L.u32p), L.ptr(tgt, L.i32p),
                                         L.ptr(ltid, L.i32p), L.ptr(lo, L.i32p), L.ptr(mid, L.i32p), L.ptr(hi1, L.i32p), C.byref(depth)))
    return code, ltid, lo, mid, hi1


_ORDER = {}


def _node_order(name, s):
    """for every node k of the library's plan, the restatement's node: both identified by (smallest transcript, number of leaves)"""
    inp = T.inputs(name)
    ti = 0 if inp["shared"] else s
    if (name, ti) not in _ORDER:
        tree = inp["trees"][ti]
        code, ltid, lo, mid, hi1 = _plan(*inp["serial"][ti])
        theirs = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(tree.k_min_tid, tree.k_size))}
        assert len(theirs) == tree.n - 1
        perm = np.array([theirs[(int(ltid[a:b].min()), int(b - a))] for a, b in zip(lo, hi1)])
        assert sorted(perm) == list(range(tree.n - 1))
        np.testing.assert_array_equal(mid - lo, tree.k_size_right[perm])  # [lo, mid) is the right child's range: tpair[..., 0]
        # bit 3 of a tour code marks the edge to the LEFT child, which reads tpair[..., 1]: one such edge per node
        edges = code[(code & 4) == 0]
        edges = edges[(edges & 3) != 1]
        assert ((edges >> 3) & 1).sum() == tree.n - 1 == len(edges) // 2
        _ORDER[(name, ti)] = perm
    return _ORDER[(name, ti)]


def _check(name, ap, lp, g, label, worst):
    inp, n = T.inputs(name), T.CASES[name][0]
    tpair, bp = ap.debug_node_terms()
    for s, ref in enumerate(T.reference(name, True)):
        perm = _node_order(name, s)
        got = dict(tp0=np.empty(n - 1), tp1=np.empty(n - 1), bp=bp[s].astype(np.float64))
        got["tp0"][perm], got["tp1"][perm] = tpair[s, :, 0], tpair[s, :, 1]
        e_node, e_sum, e_lp = T.node_gap(got, ref), T.sum_gap(got, ref), abs(float(lp[s]) - ref["lp"]) / float(T.ulp32(ref["lp"]))
        d_bp = np.abs(got["bp"] - ref["bp"])
        e_bp = float((np.maximum(d_bp - T.ulp32(ref["bp"]), 0.0) / ref["path_abs"]).max())
        d_g = np.abs(g[s].astype(np.float64) - ref["x_grad"])
        e_g = float((np.maximum(d_g - T.ulp32(ref["x_grad"]), 0.0) / T.grad_scale(ref, n)).max())
        print("%s %s s=%d: node %.3e (T %.3e)  sums %.3e (E_U %.3e)  bp %.3e  lp %.3f ulp  x_grad %.3e (T %.3e)"
              % (name, label, s, e_node, T.T_NODE, e_sum, T.E_U, e_bp, e_lp, e_g, T.T_GRAD))
        for key, v in (("node", e_node), ("sums", e_sum), ("bp", e_bp), ("lp_ulps", e_lp), ("x_grad", e_g)):
            worst[key] = max(worst.get(key, 0.0), v)
        k = int(np.argmax(np.maximum(np.abs(got["tp0"] - ref["tp0"]), np.abs(got["tp1"] - ref["tp1"])) / T.node_scale(ref)))
        where = (name, label, s, "node", k, "u", float(ref["u"][k]), "y", float(ref["y"][k]), "y_grad", float(ref["y_grad"][k]))
        assert np.isfinite(tpair[s]).all() and np.isfinite(bp[s]).all() and np.isfinite(g[s]).all(), where
        assert e_node <= T.T_NODE, where
        assert e_sum <= T.E_U, where
        assert e_bp <= T.T_NODE, (name, label, s, "leaf", int(np.argmax(d_bp / ref["path_abs"])))
        assert e_lp <= 1.0, (name, label, s, float(lp[s]), ref["lp"])
        assert e_g <= T.T_GRAD, (name, label, s, "transcript", int(np.argmax(d_g / T.grad_scale(ref, n))))


@pytest.mark.parametrize("name,variant", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_density_node_terms_and_gradient_match_f64_restatement(P, ctx, monkeypatch, name, variant):
    inp = T.inputs(name)
    for var in VARIANTS[variant]:  # (read in polee_approx_create)
        monkeypatch.setenv(var, "1")
    ap = P.RNASeqApproxLikelihood({k: inp[k] for k in ("efflen", "la_mu", "la_sigma", "la_alpha", "left_index", "right_index",
                                                       "leaf_index")}, ctx=ctx)
    worst = {}
    lp, g = ap.log_prob(inp["x"], want_grad=True)
    _check(name, ap, lp, g, variant, worst)
    # again on the same handle, a call without a gradient in between (the spine scan turns the chunk totals into offsets in place: every
    # call has to refill them); not bitwise, the sums over x end in atomics
    lp2 = ap.log_prob(inp["x"])
    lp3, g3 = ap.log_prob(inp["x"], want_grad=True)
    _check(name, ap, lp3, g3, variant + "/repeat", worst)
    for s, ref in enumerate(T.reference(name, True)):
        one = float(T.ulp32(ref["lp"]))
        assert abs(float(lp2[s]) - ref["lp"]) <= one, (name, s, float(lp2[s]), ref["lp"])
        assert abs(float(lp2[s]) - float(lp[s])) <= one and abs(float(lp3[s]) - float(lp[s])) <= one, (name, s, lp[s], lp2[s], lp3[s])
    print("WORST %s %s %s" % (variant, name, " ".join("%s=%.3e" % kv for kv in sorted(worst.items()))))


def test_node_terms_hook_rejects_null_arguments(P, ctx):
    from polee_amd import _lib as L
    inp = T.inputs("n3")
    ap = P.RNASeqApproxLikelihood({k: inp[k] for k in ("efflen", "la_mu", "la_sigma", "la_alpha", "left_index", "right_index",
                                                       "leaf_index")}, ctx=ctx)
    tp, bp = np.zeros(16, np.float64), np.zeros(16, np.float32)
    assert L.lib().polee_debug_approx_node_terms(ap._h, None, None) == 1  # POLEE_ERR_BAD_ARG
    assert L.lib().polee_debug_approx_node_terms(ap._h, L.ptr(tp, L.f64p), None) == 1
    assert L.lib().polee_debug_approx_node_terms(ap._h, None, L.ptr(bp, L.f32p)) == 1
    assert L.lib().polee_debug_approx_node_terms(None, L.ptr(tp, L.f64p), L.ptr(bp, L.f32p)) == 1

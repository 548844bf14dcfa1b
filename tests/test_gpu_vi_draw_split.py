"""The draw split of the VI loop's tree kernels (csrc/vi_fused.hpp, DrawSplit): the forward and backward kernels run a chunk's K
draws in ceil(K / DPW) workgroups of DPW draws.  The draws are independent until the update adds their gradient terms in draw
order, so every split must give the SAME BITS as DPW = K, the geometry without a split -- and that one must agree with the
oracle.  (The update kernel has no split: the hook takes only K for it.)

Shapes: n = 2 (one node), n = 513 (one 512-leaf chunk plus one leaf; at K = 8 the chunks hold 256 leaves: three of them) and
n = 1 100 (three 512-leaf chunks, five of 256 at K = 8; a forward pass of three and a half 1 024-entry chunks of the tour), on a
caterpillar (every node crosses chunks: the exported prefix rows and the chunk offsets), a balanced and a random tree (nodes
inside a chunk: the subtree sums from LDS rows).  K = 4 and K = 8 with DPW = 3 have a last group of fewer draws than DPW.

Tolerances against the oracle are those of test_gpu_parity.py::test_vi_trajectory_with_supplied_noise, for the same reason (ADAM's
first steps move a parameter by its full step whatever the gradient's size: a gradient near zero is sign-sensitive to rounding)."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_tree
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STEPS = 3


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


_samples = {}


def _sample(P, ctx, n):
    """One sample per n, shared by every case of that size: five fragments per transcript.  The bitwise comparison needs the
    sparse pass's deterministic mode, which does not cover fragments without any set structure (polee_loglik_info.stream_rows[6],
    the CSR stream, is added with float atomics): the generator's fragments share their gene's transcript sets."""
    if n not in _samples:
        if n == 2:
            import scipy.sparse as sp
            D = np.array([[3e-4, 0], [0, 5e-4], [2e-4, 7e-4], [1e-4, 0], [0, 9e-4], [6e-4, 0], [4e-4, 0]], np.float32)
            X = sp.csc_matrix(D); X.sort_indices(); X.eliminate_zeros()
            m, eff = D.shape[0], np.array([500.0, 900.0], np.float32)
            colptr, rowval, nzval = (X.indptr + 1).astype(np.uint32), (X.indices + 1).astype(np.uint32), X.data.astype(np.float32)
        else:
            from tools import synth
            smp = synth.make_sample(n, 5 * n, 4.0, 17)
            m, eff = smp["m"], smp["effective_lengths"]
            colptr, rowval, nzval = synth.to_csc(smp)
        s = P.RNASeqSample(m, n, colptr, rowval, nzval, eff, ctx=ctx)
        rows = s.info["stream_rows"] if isinstance(s.info, dict) else s.info()["stream_rows"]
        assert rows[6] <= (1 if n == 2 else 0), rows  # (n = 2: one such fragment, one add per transcript: nothing to reorder)
        _samples[n] = (s, O.Sample(m, n, colptr, rowval, nzval), eff)
    return _samples[n]


def _offered(K):
    """The draw splits the hook offers for K draws: K itself, and 3, 2, 1 where they are below it."""
    return [K] + [d for d in (3, 2, 1) if d < K]


def _set_split(fit, dpw):
    from polee_amd import _lib as L
    L.check(L.lib().polee_vi_debug_set_draw_split(fit._h, C.c_int32(dpw), C.c_int32(dpw), C.c_int32(0)), fit.ctx._h)


def _sixteen_decades(parents, js, n, rng):
    """The parameters of test_gpu_parity.py::test_vi_subtree_sums_across_chunks_and_sixteen_decades for a caterpillar: y ~ 0.9975
    towards the larger subtree (the chain's u decays slowly), noise on top, and forty extreme nodes for tiny subtrees."""
    from polee_amd import _lib as L
    N = 2 * n - 1
    code = np.zeros(3 * n - 2, np.uint32); tgt = np.zeros(3 * n - 2, np.int32); ltid = np.zeros(n, np.int32)
    lo, mid, hi1 = (np.zeros(n - 1, np.int32) for _ in range(3))
    depth = C.c_int32()
    pp, jj = np.ascontiguousarray(parents, np.int32), np.ascontiguousarray(js, np.int32)
    L.check(L.lib().polee_debug_ptt_plan(L.ptr(pp, L.i32p), L.ptr(jj, L.i32p), N, L.ptr(code, L.u32p), L.ptr(tgt, L.i32p),
                                         L.ptr(ltid, L.i32p), L.ptr(lo, L.i32p), L.ptr(mid, L.i32p), L.ptr(hi1, L.i32p), C.byref(depth)))
    left_bigger = (hi1 - mid) > (mid - lo)  # y multiplies the LEFT child (ptt.jl:147)
    mu = (np.where(left_bigger, 6.0, -6.0) + rng.normal(0, 0.5, n - 1)).astype(np.float32)
    mu[rng.integers(0, n - 1, 40)] = rng.choice([-18.0, 18.0], 40).astype(np.float32)
    omega = rng.normal(-1.5, 0.3, n - 1).astype(np.float32)
    alpha = rng.normal(0, 0.2, n - 1).astype(np.float32)
    return mu, omega, alpha


def _run(P, s, t, K, dpw, z0=None, start=None):
    """STEPS iterations with the draw split dpw in the forward and the backward kernel, then the gradients of the next iteration's draws (the hook's
    outputs).  z0 = None: the device's generator and the gradient-only loop (the update kernel draws the next iteration's samples);
    z0 given: the caller's noise and the loop that also records the ELBO."""
    fit = P.LikelihoodApproximationFit(s, t, num_steps=STEPS + 1, num_mc_samples=K, seed=77, deterministic=True, z0=z0,
                                       gradonly=z0 is None)
    _set_split(fit, dpw)
    if start is not None:
        fit.set_params(*start)
    fit.run(STEPS)
    fit.sync()
    mu, om, al = fit.params()
    res = dict(mu=mu, omega=om, alpha=al)
    if z0 is not None:
        res["elbo"], res["lp_mean"] = fit.trace()
    for key, val in fit.eval_gradients().items():
        res["next_" + key] = val
    return res


@pytest.mark.parametrize("K", [1, 4, 6, 8])
@pytest.mark.parametrize("n", [2, 513, 1100])
@pytest.mark.parametrize("kind", ["spine", "balanced", "random"])
def test_draw_split_is_bitwise_the_unsplit_step(P, ctx, kind, n, K):
    s, so, eff = _sample(P, ctx, n)
    rng = np.random.default_rng(4321)
    parents, js = random_tree(n, rng, kind)
    t = P.PolyaTreeTransform(parents, js, ctx=ctx)
    # the caterpillar starts from parameters that spread the leaves over more than sixteen decades (the crossing-node path with
    # tiny subtrees beside large ones); the other trees from the fit's own initial values
    start = _sixteen_decades(parents, js, n, rng) if kind == "spine" else None
    z0 = O.randn((STEPS + 1) * K * (n - 1), 3)
    base = {"rng": _run(P, s, t, K, K, None, start), "z0": _run(P, s, t, K, K, z0, None)}
    if start is not None and n > 2:
        xs = base["rng"]["next_xs"]
        assert xs.min() <= 1.001e-10 and xs.max() > 1e-3, (xs.min(), xs.max())  # (xs is clamped at 1e-10: u goes far below)
    for noise, res in base.items():
        print("%s n=%d K=%d %s: non-finite values in %s" % (kind, n, K, noise, [k for k, v in res.items() if not np.isfinite(v).all()]))
        assert all(np.isfinite(res[k]).all() for k in ("mu", "omega", "alpha", "next_y_grad", "next_mu_grad", "next_omega_grad", "next_alpha_grad"))
    # DPW = K against the oracle: the trajectory's tolerances
    ref = O.approximate_likelihood(so, O.PTT(parents, js), eff, num_steps=STEPS, num_mc=K, z0=z0[:STEPS * K * (n - 1)], gradonly=False)
    got = base["z0"]
    for key in ("mu", "omega", "alpha"):
        err = np.abs(got[key] - ref[key]) / (1 + np.abs(ref[key]))
        print("%s n=%d K=%d %s: max err %.3g, within 2e-4: %.4f" % (kind, n, K, key, err.max(), (err <= 2e-4).mean()))
    for key in ("lp_mean", "elbo"):
        print("%s n=%d K=%d %s: max rel err %.3g" % (kind, n, K, key, np.abs(got[key][:STEPS] / ref[key] - 1).max()))
    for key in ("mu", "omega", "alpha"):
        ok = np.abs(got[key] - ref[key]) <= 2e-4 * (1 + np.abs(ref[key]))
        assert ok.mean() >= 0.99, (key, ok.mean())
    np.testing.assert_allclose(got["lp_mean"][:STEPS], ref["lp_mean"], rtol=1e-5)
    np.testing.assert_allclose(got["elbo"][:STEPS], ref["elbo"], rtol=1e-5)
    # every other split the hook offers against DPW = K: the same bits, parameters and the hook's gradient outputs.  (Not compared:
    # the log-determinant of the sampling step and the ELBO that contains it -- vi_sample_k_kernel adds its workgroups' sums
    # with double atomics, in whatever order they finish, with or without a split.)
    for dpw in _offered(K)[1:]:
        for noise, zz, st in (("rng", None, start), ("z0", z0, None)):
            res = _run(P, s, t, K, dpw, zz, st)
            for key, want in base[noise].items():
                if key in ("next_ladj", "elbo"):
                    continue
                assert res[key].tobytes() == want.tobytes(), (dpw, noise, key, int((res[key] != want).sum()))


def test_hook_rejects_a_split_that_is_not_instantiated(P, ctx):
    s, _, _ = _sample(P, ctx, 2)
    t = P.PolyaTreeTransform(np.array([0, 1, 1], np.int32), np.array([0, 1, 2], np.int32), ctx=ctx)
    fit = P.LikelihoodApproximationFit(s, t, num_steps=1, num_mc_samples=6)
    for bad in (4, 5, 7, -1):
        with pytest.raises(Exception):
            _set_split(fit, bad)
    _set_split(fit, 0)  # back to the library's own choice
    from polee_amd import _lib as L
    with pytest.raises(Exception):  # (the update kernel: all draws of a node on one lane)
        L.check(L.lib().polee_vi_debug_set_draw_split(fit._h, C.c_int32(0), C.c_int32(0), C.c_int32(3)), fit.ctx._h)
    L.check(L.lib().polee_vi_debug_set_draw_split(fit._h, C.c_int32(0), C.c_int32(0), C.c_int32(6)), fit.ctx._h)

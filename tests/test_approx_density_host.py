"""CPU tests of tests/approx_density_restatement.py, the float64 restatement tests/test_gpu_approx_density.py holds the density kernels
(polee_amd/csrc/approx.hip) to: it agrees with the oracle, its inputs satisfy what the checks presuppose, the stored tolerances are
the ones the restatement itself measures, and three mutants -- a double-double prefix without its low word, a tour scan in plain
doubles, a crossing node without its chunk offset -- miss those tolerances by a wide margin.  No GPU."""
import numpy as np
import pytest

import approx_density_restatement as T
from conftest import random_tree
from oracle import oracle as O


@pytest.mark.parametrize("shared", [False, True])
def test_restatement_matches_the_oracle_on_benign_inputs(shared):
    """The inputs of test_gpu_parity.py::test_approx_logprob_and_gradient_match_oracle.  lp: the oracle keeps InvHSB's running
    Float32 accumulator of -log u (600 roundings at |ladj| of a few thousand, some 1e-6 of lp), which the restatement does not."""
    rng = np.random.default_rng(21)
    n, S = 600, 3
    trees = [random_tree(n, rng) for _ in range(1 if shared else S)]
    idx = [O.make_inverse_ptt_params(*tr) for tr in trees]
    L_, R_, F_ = (np.stack([i[j] for i in idx]) for j in range(3))
    x = rng.normal(0, 1.5, size=(S, n)).astype(np.float32)
    eff = rng.uniform(200, 3000, size=(S, n)).astype(np.float32)
    mu = rng.normal(0, 1, size=(S, n - 1)).astype(np.float32)
    sigma = np.exp(rng.normal(-1, 0.3, size=(S, n - 1))).astype(np.float32)
    alpha = rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32)
    lpo, go = O.approx_log_prob(x, eff, mu, sigma, alpha, L_, R_, F_, want_grad=True)
    for s in range(S):
        t = T.Tree(*trees[0 if shared else s])
        for a, b in zip(t.index_arrays(), (L_, R_, F_)):
            np.testing.assert_array_equal(a, b[0 if shared else s])
        r = T.density(t, x[s], eff[s], mu[s], sigma[s], alpha[s], f32_steps=True)
        np.testing.assert_allclose(r["lp"], lpo[s], rtol=1e-5)
        np.testing.assert_allclose(r["x_grad"], go[s], rtol=1e-4, atol=1e-5 * np.abs(go[s]).max())
        assert r["u"].max() == pytest.approx(1.0, abs=1e-6) and (r["path_abs"] >= np.abs(r["bp"])).all()


@pytest.mark.parametrize("name", list(T.CASES))
def test_inputs_satisfy_what_the_checks_presuppose(name):
    """No q is 0 or subnormal as Float32, no y within 1e-9 of 0 or 1, the smallest node sum as small as the case is there for
    (T.input_conditions); z stays O(1); and the Float32 steps move lp by at most a tenth of a Float32 ulp, so that 'lp within one ulp'
    is half an ulp of the final cast plus noise."""
    fig = T.input_conditions(name)
    assert max(f["zmax"] for f in fig) < 12.0, fig
    for r32, r64 in zip(T.reference(name, True), T.reference(name, False)):
        assert abs(r32["lp"] - r64["lp"]) <= 0.1 * float(T.ulp32(r64["lp"])), (name, r32["lp"], r64["lp"])
        assert T.sum_gap(r32, r64) <= 0.5 * T.E_U


def test_shapes_cover_the_chunk_edges():
    """What the shapes are there for, from the restatement's own leaf order: a tree with no crossing node, a second chunk of one
    leaf, n a multiple of the chunk, more than 256 crossing nodes (two blocks of them), boundaries exactly on chunk multiples, chunks
    in which no node starts, every node starting in chunk 0, every node ending at n, and trees of one handle that differ."""
    cross = {name: [len(T.crossing_nodes(t)) for t in T.inputs(name)["trees"]] for name in T.CASES}
    assert cross["random511"] == [0] and cross["random512"] == [0] and cross["n2"] == [0]
    assert cross["spine3000"][0] > 2 * 256 and cross["spine1100"][0] > 256
    assert len(set(cross["mixed1536"])) == 3 and max(cross["mixed1536"]) > 256 > min(cross["mixed1536"])
    t = T.inputs("random513")["trees"][0]
    assert cross["random513"][0] >= 1 and t.n == T.CHUNK + 1
    for name in ("balanced1024", "balanced2048"):
        t = T.inputs(name)["trees"][0]
        assert (t.k_hi[T.crossing_nodes(t)] % T.CHUNK == 0).all() and (t.k_mid[T.crossing_nodes(t)] % T.CHUNK == 0).all()
    lo, hi = T.inputs("spine_lo1537")["trees"][0], T.inputs("spine_hi1537")["trees"][0]
    assert (lo.k_lo == 0).all() and (hi.k_hi == hi.n).all() and len(set(hi.k_lo)) == hi.n - 1
    starts = set((T.inputs("spine_lo1537")["trees"][0].k_lo // T.CHUNK).tolist())
    assert starts == {0}  # (chunks 1.. of that tree: no node starts there)
    assert T.CASES["mixed1536"][0] % T.CHUNK == 0 and T.CASES["balanced1024"][0] % T.CHUNK == 0


def test_stored_tolerances_are_what_the_restatement_measures():
    """G_NODE and G_GRAD are the gaps between the Float32-step and the all-Float64 restatement, T = 8 G.  (Within a factor of two:
    NumPy's Float32 exp, log, sinh, ... differ by an ulp between its SIMD builds, and a maximum over 27 000 nodes moves with that.)"""
    g_node, g_grad, per = T.measure_gaps()
    assert T.G_NODE / 2 <= g_node <= 2 * T.G_NODE, (g_node, per)
    assert T.G_GRAD / 2 <= g_grad <= 2 * T.G_GRAD, (g_grad, per)
    assert T.T_NODE == 8 * T.G_NODE and T.T_GRAD == 8 * T.G_GRAD


def _mutant_misses():
    out = {}
    for name in T.CASES:
        if T.CASES[name][0] <= T.CHUNK:
            continue
        refs = T.reference(name, True)
        m = {w: [T.mutant(name, s, w) for s in range(len(refs))] for w in "abc"}
        out[name] = dict(umin=min(float(r["u"].min()) for r in refs),
                         a=max(T.node_gap(g, r) for g, r in zip(m["a"], refs)),
                         a_sum=max(T.sum_gap(g, r) for g, r in zip(m["a"], refs)),
                         b=max(T.bp_gap(g, r) for g, r in zip(m["b"], refs)),
                         c=max(T.node_gap(g, r) for g, r in zip(m["c"], refs)),
                         c_sum=max(T.sum_gap(g, r) for g, r in zip(m["c"], refs)))
    return out


def test_the_mutants_miss_the_tolerances_tenfold():
    """(a) node sums from a plain-double prefix, (b) bp from a plain-double prefix over the tour, (c) one crossing node without its
    chunk offset: each misses T_NODE by 10x or more on some case, (a) on every case whose smallest node sum is <= 1e-15.  The
    derived bound on the node sums (E_U) is far sharper: (a) misses it tenfold wherever a node sum below 1e-11 lies behind a prefix, (c) everywhere."""
    miss = _mutant_misses()
    for w in "abc":
        assert max(v[w] for v in miss.values()) >= 10 * T.T_NODE, (w, miss)
    tiny = [name for name, v in miss.items() if v["umin"] <= 1e-15]
    assert len(tiny) >= 5
    for name in tiny:
        assert miss[name]["a"] >= 10 * T.T_NODE, (name, miss[name])
    for name, v in miss.items():
        assert v["c_sum"] >= 10 * T.E_U, (name, v)
        if v["umin"] <= 1e-11 and name != "spine_lo1537":  # (every node of that tree starts at position 0: nothing cancels)
            assert v["a_sum"] >= 10 * T.E_U, (name, v)

"""CPU checks of tests/tree_ops_restatement.py, the float64 reference that tests/test_gpu_tree_saturation.py and
tests/test_gpu_tree_ops_large.py hold the tree kernels to: the restatement agrees with the C oracle on every saturated case (two
independent statements of the reference), its float64 values are good to a tenth of every bound they are used with, the constant of
the InvHSB gradient's bound still holds, and the part-B sizes see the three scan faults they exist for.  No GPU."""
import numpy as np
import pytest

import tree_ops_restatement as R
from oracle import oracle as O

F32_FLOOR = np.float32(1e-16)
HAS_LD = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def _floor_set(x, floor=F32_FLOOR):
    return set(np.flatnonzero(np.asarray(x) == floor).tolist())


def _check_live(got, ref, rtol, atol, floor=F32_FLOOR):
    """the floor sets are equal, the other leaves within the bound; returns the number of live leaves"""
    assert _floor_set(got, floor) == _floor_set(ref, floor)
    live = np.asarray(ref) != floor
    np.testing.assert_allclose(np.asarray(got)[live], np.asarray(ref)[live], rtol=rtol, atol=atol)
    return int(live.sum())


def test_case_list_has_every_placement_where_the_issue_needs_it():
    cases = set(R.sat_cases())
    for kind, n in (("fixture", 313), ("random", 1100), ("spine", 1100), ("balanced", 1024)):
        for name in R.PLACEMENTS:
            assert (kind, n, name) in cases, (kind, n, name)
    assert ("random", 2, "root") in cases and ("random", 3, "one_y1") in cases
    # the two internal-child variants are what they say
    for kind, n in R.SAT_TREES[:4]:
        _, pl, where, _ = R.sat_inputs(kind, n, "internal_cross_chunk")
        (k, y), = where.items()
        s = 0 if y == 1.0 else 1
        last = (pl["TL"] - 1) // R.CHUNK
        assert pl["TL"] % R.CHUNK and pl["enter"][k, s] // R.CHUNK < pl["exit"][k, s] // R.CHUNK == last
        assert (last, pl["TL"]) == (6, 3298) or n != 1100
        assert (pl["typ"][pl["exit"][k, s] + 1:] == 2).any()  # leaves follow the EXIT: a poisoned prefix would show
        _, pl, where, _ = R.sat_inputs(kind, n, "internal_same_chunk")
        (k, y), = where.items()
        s = 0 if y == 1.0 else 1
        assert 0 <= pl["enter"][k, s] // R.CHUNK == pl["exit"][k, s] // R.CHUNK
        assert (pl["typ"][pl["exit"][k, s] + 1:] == 2).any()
    _, pl, where, _ = R.sat_inputs("random", 1100, "leaf_child")
    (k, y), = where.items()
    assert pl["enter"][k, 0 if y == 1.0 else 1] < 0


@pytest.mark.parametrize("kind,n,name", R.sat_cases())
def test_restatement_agrees_with_the_oracle_on_saturated_nodes(kind, n, name):
    t, pl, where, ys = R.sat_inputs(kind, n, name)
    to = O.PTT(t.parents, t.js)
    l, r, f = t.index_arrays()
    rng = np.random.default_rng(n)
    # transform with exact 0.0 / 1.0
    y = R.saturate(ys[0], where)
    xs, ladj, u = R.transform(t, y)
    xo, lo = to.transform(y, True)
    live = _check_live(xs, xo, 3e-7, 0)
    assert live >= 1 and abs(float(xs.astype(np.float64).sum()) - 1) < 1e-4
    assert R.ladj_matches(float(ladj), lo)
    any_internal_dead = any(pl["enter"][k, 0 if v == 1.0 else 1] >= 0 for k, v in where.items())
    assert np.isneginf(lo) == any_internal_dead
    # hsb with logits of +-40 and +-100
    for big in (40.0, 100.0):
        logit = R.saturated_logits(ys[0], where, big)
        xh, xho = R.hsb(t, logit), O.hsb(logit, l, r, f)[0]
        assert _check_live(xh, xho, 1e-6, 0, np.float32(0)) >= 1 and abs(float(xh.astype(np.float64).sum()) - 1) < 1e-4
        if big == 100.0:  # (the double's logistic is 1 from 36.8 on but 0 only where expf overflows, below -88.7)
            assert _floor_set(xh, 0) == _floor_set(xs)  # the same leaves die
    # sampler draw, initial values and the TF sampler with mu of +-17, +-30, -120 on the chosen nodes
    mu, sigma, alpha, z0, eff = R.sampler_params(n - 1, where, rng)
    xd, xdo = R.sampler_draw(t, mu, sigma, alpha, z0), O.sampler_draw(to, mu, sigma, alpha, z0)
    assert _check_live(xd, xdo, 2e-5, 1e-30) >= 1 and abs(float(xd.astype(np.float64).sum()) - 1) < 1e-4
    assert _floor_set(xs) <= _floor_set(xd)  # what exact saturation kills, the sampler's saturated logistic kills
    np.testing.assert_allclose(R.x0_draw(t, mu, sigma, alpha, eff, z0), O.x0_draw(to, mu, sigma, alpha, eff, z0), rtol=2e-5, atol=1e-30)
    mu = R.sampler_params(n - 1, where, rng, ones=(40.0, 100.0))[0]  # (the op's logistic is a double's: 17 and 30 leave it below 1)
    xt, xto = R.tf_sampler(t, mu, sigma, alpha, eff, z0), O.tf_sampler(z0, eff, mu, sigma, alpha, l, r, f)[0]
    assert _check_live(xt, xto, 1e-4, 1e-16) >= 1 and _floor_set(xs) <= _floor_set(xt)


@pytest.mark.parametrize("kind,n", R.SAT_TREES[:4])
def test_near_saturated_sampler_inputs_keep_their_leaves_above_the_floor(kind, n):
    """mu = -17 and -30 on the nodes tests/test_gpu_tree_saturation.py gives the device: live in the oracle and the restatement"""
    t, _ = R.sat_tree(kind, n)
    to = O.PTT(t.parents, t.js)
    mu, sigma, alpha, z0, tids = R.near_saturated_sampler(kind, n)
    for d in range(len(z0)):
        xo = O.sampler_draw(to, mu, sigma, alpha, z0[d])
        assert (xo[tids] > F32_FLOOR).all() and (xo[tids] < 1e-6).all()
        np.testing.assert_allclose(R.sampler_draw(t, mu, sigma, alpha, z0[d]), xo, rtol=2e-5, atol=1e-30)


def test_large_and_negative_logits_that_do_not_saturate_stay_live():
    """mu = -17 and -30 leave y > 0 in Float32 (1 / (1 + e^17) = 4e-8): the left side is tiny, not dead -- the restatement and the
    oracle agree on it to the sampler's tolerance"""
    t, _, _, _ = R.sat_inputs("fixture", 313, "one_y0")
    to = O.PTT(t.parents, t.js)
    rng = np.random.default_rng(3)
    mu, sigma, alpha, z0, _ = R.sampler_params(312, {}, rng)
    mu[[5, 40, 100, 200]] = (-17.0, -30.0, 17.0, 30.0)
    sigma[[5, 40, 100, 200]] = 1e-3
    np.testing.assert_allclose(R.sampler_draw(t, mu, sigma, alpha, z0), O.sampler_draw(to, mu, sigma, alpha, z0), rtol=2e-5, atol=1e-30)


# ---- part B ------------------------------------------------------------------------------------------------------------------------

SMALL_LARGE = [c for c in R.LARGE_CASES if c[1] < 100000]


@pytest.mark.parametrize("kind,n", R.LARGE_CASES)
def test_float64_reference_is_good_to_a_tenth_of_every_bound(kind, n):
    """the gap between the float64 and the long double run of the restatement, in units of the bound each quantity is used with"""
    if not HAS_LD:
        pytest.skip("np.longdouble is float64 here: no higher precision to compare the reference with")
    a, b = R.large_reference(kind, n), R.large_reference(kind, n, R.LD)
    got = {k: a[k] for k in ("xs", "ladj", "yg", "yg0", "inv_y", "inv_ladj_jl", "inv_ladj_tf", "hsb", "bp")}
    # xs and hsb are compared before their rounding to Float32
    got["xs"], got["hsb"] = a["u_leaf"], a["hsb_u"]
    ref = dict(b)
    ref["xs"], ref["hsb"] = b["u_leaf"], b["hsb_u"]
    err = R.scaled_errors(kind, n, got, ref)
    print(kind, n, {k: "%.2e" % v for k, v in err.items()})
    assert all(v <= 0.1 for v in err.values()), err
    assert np.max(np.abs(a["logu"] - b["logu"])) < 1e-12
    assert a["u_leaf"].min() > 1e-30  # nothing near underflow


def test_c_path_constant_still_holds():
    if not HAS_LD:
        pytest.skip("np.longdouble is float64 here")
    c = R.measure_c_path()
    print("measured c = %.3e" % c)
    assert c <= R.C_PATH_MEASURED and R.C_PATH == 10 * R.C_PATH_MEASURED


@pytest.mark.parametrize("kind,n", R.LARGE_CASES)
def test_device_algorithm_in_float64_meets_the_bounds(kind, n):
    """the three-phase scan as the device runs it, emulated on the host, passes: the mutants below fail for what they change"""
    err = R.scaled_errors(kind, n, R.emulate_device(kind, n))
    assert all(v <= 1 for v in err.values()), err


def _breaks(kind, n, mutant):
    return not all(v <= 1 for v in R.scaled_errors(kind, n, R.emulate_device(kind, n, mutant)).values())  # (NaN breaks too)


def test_mutant_spine_that_omits_a_threads_first_total():
    for kind, n in R.LARGE_CASES:
        assert _breaks(kind, n, "spine_first_total") == (n > 43691), (kind, n)


def test_mutant_leaf_prefix_without_its_low_word():
    assert any(_breaks(kind, n, "no_low_word") for kind, n in SMALL_LARGE)


def test_mutant_dropped_last_element_of_a_partial_chunk():
    for kind in ("random", "balanced", "spine"):
        assert _breaks(kind, 131073, "partial_tail")
    assert not _breaks("random", 131072, "partial_tail")  # (its tour's last entry, alone in a chunk's tail, is the root's EXIT)

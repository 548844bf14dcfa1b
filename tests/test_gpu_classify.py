"""-m gpu: RNASeqLogisticRegression (polee_amd/classify.py, csrc/classify.hip; models/polee_classify.py:13-114) against the NumPy
float64 restatement tests/classify_restatement.py.

The restatement is fed the DEVICE'S OWN draws (polee_approx_sample with the same z0 slice, one call per draw; the sampler's parity with
the oracle is covered by tests/test_gpu_parity.py), so a wrong z0 slice, draw count or seed rule is an O(1) error.

Tolerances.  Loss: 1e-5 |loss_ref| + 2 S B with B = 4e-7 max_{s,c} sum_j |lx[s][j] w[j][c]| + 1e-6: the f32 FMA-chain error of a logit
(3.5e-7 sum |a b| at chain length 4096, rounded up) plus one ulp of logf at |lx| ~ 10, through a softmax whose derivative is at most 1.
Gradients: the convention of tests/test_gpu_regression.py, an entry within 1e-2 relative to |ref| + 2e-3 max |g| of its block.
Probabilities: 2 B.  Adam: against the device's own gradients, |p_dev - p_host| <= 1e-5 lr_t + 6e-8 |p|.  No multi-step trajectory is
compared with a float64 one: m / (sqrt(v) + eps) is +-1 on the first step whatever the gradient's size and the L1 term jumps at 0, so
rounding-level gradient differences grow into O(lr) parameter differences.

Worst observed ratios (MI355X): profiles/classify_parity_margins.txt.
"""
import ctypes as C

import numpy as np
import pytest

import classify_restatement as T
from conftest import random_tree
from oracle import oracle as O

pytestmark = pytest.mark.gpu

L1 = 1e-3


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def ctx(P):
    return P.Context(0)


_PROBLEMS = {}


def _problem(P, ctx, S, n):
    """random trees, per-sample parameters (as _problem of tests/test_gpu_pca.py); built once per shape"""
    if (S, n) not in _PROBLEMS:
        rng = np.random.default_rng(1000 * S + n)
        trees = [random_tree(n, rng) for _ in range(S)]
        idx = [O.make_inverse_ptt_params(*tr) for tr in trees]
        L_, R_, F_ = (np.stack([i[j] for i in idx]) for j in range(3))
        vars_ = dict(efflen=rng.uniform(200, 3000, size=(S, n)).astype(np.float32),
                     la_mu=rng.normal(0, 1, size=(S, n - 1)).astype(np.float32),
                     la_sigma=np.exp(rng.normal(-1, 0.3, size=(S, n - 1))).astype(np.float32),
                     la_alpha=rng.normal(0, 0.3, size=(S, n - 1)).astype(np.float32), left_index=L_, right_index=R_, leaf_index=F_)
        _PROBLEMS[(S, n)] = P.RNASeqApproxLikelihood(vars_, ctx=ctx)
    return _PROBLEMS[(S, n)]


def _draws(ap, z0):
    """the device's own draws for z0 [D][S][n-1], as log expression in float64"""
    return np.stack([np.log(ap.sample(z0=z.copy()).astype(np.float64)) for z in z0])


def _params(rng, lx0, n, k, zeros=0):
    w = rng.normal(0, 0.1, size=(n, k)).astype(np.float32)
    if zeros:
        w.reshape(-1)[rng.choice(n * k, zeros, replace=False)] = 0.0
    xb = (lx0.mean(axis=0) + rng.normal(0, 0.3, size=n)).astype(np.float32)
    zb = rng.normal(0, 0.5, size=k).astype(np.float32)
    return w, xb, zb


def _labels(rng, S, k):
    return np.eye(k, dtype=np.float32)[rng.integers(0, k, size=S)]


def _B(lx, w):
    return 4e-7 * np.einsum("dsj,jc->dsc", np.abs(lx), np.abs(w.astype(np.float64))).max() + 1e-6


def _check(tag, loss, grads, ref, S, B):
    loss_o, refs = ref[0], ref[1:]
    tol = 1e-5 * abs(loss_o) + 2 * S * B
    worst = [abs(loss - loss_o) / tol]
    for g, r in zip(grads, refs):
        worst.append(float((np.abs(g - r) / (np.abs(r) + 2e-3 * np.abs(r).max())).max()) / 1e-2)
    print("MARGIN %s loss %.6g ref %.6g  used: loss %.3g g_w %.3g g_x_bias %.3g g_z_bias %.3g" % ((tag, loss, loss_o) + tuple(worst)))
    assert worst[0] <= 1.0, (loss, loss_o, tol)
    for name, u in zip(("g_w", "g_x_bias", "g_z_bias"), worst[1:]):
        assert u < 1.0, (name, u)


# (n, S, k, D, loss_scale): n = 130, 150 are no multiple of 64 or of the logits kernel's chunk (128 transcripts, one wave; four chunks
# per workgroup); 1100 = 9 chunks in 3 workgroups, the last chunk and the last workgroup ragged; k = 2, 3, 6, 16 run the kernels'
# four widths (2, 4, 8, 16 classes), k = 3 and 6 with padding
CASES = [(130, 1, 2, 1, 1.0), (150, 5, 3, 5, 0.7), (130, 5, 16, 1, 1.0), (150, 1, 16, 5, 2.5), (150, 5, 2, 5, 1.0), (130, 1, 3, 1, 0.7),
         (150, 5, 6, 1, 1.0), (1100, 5, 3, 5, 1.0), (1100, 5, 16, 1, 0.7)]


@pytest.mark.parametrize("n,S,k,D,loss_scale", CASES)
def test_loss_and_gradients_match_restatement(P, ctx, n, S, k, D, loss_scale):
    rng = np.random.default_rng(81)
    ap = _problem(P, ctx, S, n)
    z0 = rng.normal(size=(D, S, n - 1)).astype(np.float32)
    lx = _draws(ap, z0)
    w, xb, zb = _params(rng, lx[0], n, k)
    y = _labels(rng, S, k)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx, draws_per_step=D, loss_scale=loss_scale)
    clf.set_params(w, xb, zb)
    for a, b in zip(clf.get_params(), (w, xb, zb)):
        np.testing.assert_array_equal(a, b)
    loss, g_w, g_xb, g_zb = clf.loss_and_gradients(S, n, ap, y, z0=z0)
    ref = T.loss_and_gradients(w, xb, zb, lx, y, L1, loss_scale)
    _check("draws n=%d S=%d k=%d D=%d ls=%g" % (n, S, k, D, loss_scale), loss, (g_w, g_xb, g_zb), ref, S, _B(lx, w))


@pytest.mark.parametrize("n,S,k,loss_scale", [(150, 5, 3, 0.7), (130, 70, 5, 1.0), (1100, 3, 16, 1.0)])
def test_point_path_matches_restatement(P, ctx, n, S, k, loss_scale):
    """x is log expression already; S = 70 needs two of the gradient kernel's 64-sample tiles"""
    rng = np.random.default_rng(82)
    x = (rng.normal(-np.log(n), 1.5, size=(1, n)) + rng.normal(0, 0.4, size=(S, n))).astype(np.float32)
    lx = x.astype(np.float64)[None]
    w, xb, zb = _params(rng, lx[0], n, k)
    y = _labels(rng, S, k)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx, loss_scale=loss_scale)
    clf.set_params(w, xb, zb)
    loss, g_w, g_xb, g_zb = clf.loss_and_gradients(x=x, z_true=y)
    ref = T.loss_and_gradients(w, xb, zb, lx, y, L1, loss_scale)
    _check("points n=%d S=%d k=%d ls=%g" % (n, S, k, loss_scale), loss, (g_w, g_xb, g_zb), ref, S, _B(lx, w))
    probs = clf.predict(x)
    assert np.abs(probs - T.predict(w, xb, zb, lx)).max() <= 2 * _B(lx, w)
    clf.init_bias(x)
    np.testing.assert_allclose(clf.get_params()[1], lx[0].mean(axis=0), rtol=1e-6)


@pytest.mark.parametrize("n,S,k", [(150, 5, 3), (1100, 5, 16)])
def test_exact_facts_at_zero_parameters(P, ctx, n, S, k):
    rng = np.random.default_rng(83)
    ap = _problem(P, ctx, S, n)
    y = _labels(rng, S, k)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx)
    for a in clf.get_params():
        assert not a.any()  # (all three start at zero, polee_classify.py:18-20)
    loss, g_w, g_xb, g_zb = clf.loss_and_gradients(S, n, ap, y, seed=3)
    assert abs(loss - S * np.log(k)) <= 1e-6 * S * np.log(k)
    assert not g_xb.any()  # (w = 0)
    np.testing.assert_allclose(g_zb, (1.0 / k - y).sum(axis=0), atol=1e-6)
    trace = clf.fit_steps_sample(S, n, ap, y, 2, seed=3)
    assert abs(trace[0] - S * np.log(k)) <= 1e-6 * S * np.log(k)
    x = np.log(ap.sample(seed=4))
    clf2 = P.RNASeqLogisticRegression(k, n, ctx=ctx)
    w, trace2 = clf2.fit(x, y, 2, return_trace=True)
    assert abs(trace2[0] - S * np.log(k)) <= 1e-6 * S * np.log(k) and w.shape == (n, k)


@pytest.mark.parametrize("n,S,k,D", [(150, 5, 3, 2), (1100, 5, 16, 1)])
def test_adam_against_the_devices_own_gradients(P, ctx, n, S, k, D):
    """three single steps: Adam's form, the sign convention of the L1 term, sign(0) = 0 and the step clock, without any sensitivity to
    the rounding of the gradients"""
    rng = np.random.default_rng(84)
    lr, steps = 1e-2, 3
    ap = _problem(P, ctx, S, n)
    z0 = rng.normal(size=(steps, D, S, n - 1)).astype(np.float32)
    w, xb, zb = _params(rng, _draws(ap, z0[0, :1])[0], n, k, zeros=7)
    y = _labels(rng, S, k)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx, draws_per_step=D, learning_rate=lr)
    clf.set_params(w, xb, zb)
    m, v = [0.0] * 3, [0.0] * 3
    worst = arith = 0.0
    for t in range(1, steps + 1):
        before = clf.get_params()
        loss, *grads = clf.loss_and_gradients(S, n, ap, y, z0=z0[t - 1])
        if t == 1:
            # the L1 term on its own: the same evaluation without a penalty differs by l1 sign(w) -- to the rounding of the f32 sum
            # g + l1 sign(w), half an ulp of |g| -- and by nothing at all where w = 0; the loss differs by l1 sum |w|
            zero = before[0] == 0
            assert zero.sum() == 7
            plain = P.RNASeqLogisticRegression(k, n, ctx=ctx, draws_per_step=D, l1_penalty=0.0)
            plain.set_params(*before)
            loss0, g0 = plain.loss_and_gradients(S, n, ap, y, z0=z0[0])[:2]
            d = grads[0].astype(np.float64) - g0
            assert (d[zero] == 0).all()
            assert (np.abs(d - L1 * np.sign(before[0])) <= 1.2e-7 * (np.abs(g0) + L1)).all()
            assert abs((loss - loss0) - L1 * np.abs(before[0].astype(np.float64)).sum()) <= 2.4e-7 * abs(loss)
        trace = clf.fit_steps_sample(S, n, ap, y, 1, z0=z0[t - 1])
        assert trace[0] == np.float32(loss)  # (the same kernels in the same order)
        after = clf.get_params()
        lr_t = lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        for i in range(3):
            host, m[i], v[i] = T.adam_step(before[i], grads[i], m[i], v[i], t, lr)
            err = np.abs(after[i].astype(np.float64) - host)
            tol = 1e-5 * lr_t + 6e-8 * np.abs(host)
            worst = max(worst, float((err / tol).max()))
            arith = max(arith, float(((err - 6e-8 * np.abs(host)) / (1e-5 * lr_t)).max()))  # (beyond the store's half ulp)
            assert (err <= tol).all(), (t, i, float((err / tol).max()))
            assert np.abs(after[i] - before[i]).max() > 0.5 * lr_t  # (the step is far above the rounding of p)
    print("MARGIN adam n=%d S=%d k=%d D=%d used %.3g of the bound; beyond the half ulp of the store %.3g of 1e-5 lr_t"
          % (n, S, k, D, worst, max(arith, 0.0)))


def test_reproducibility_is_bitwise(P, ctx):
    rng = np.random.default_rng(85)
    n, S, k, D = 150, 5, 3, 2
    ap = _problem(P, ctx, S, n)
    y = _labels(rng, S, k)
    lx0 = np.log(ap.sample(seed=1).astype(np.float64))
    w, xb, zb = _params(rng, lx0, n, k)

    def fresh():
        c = P.RNASeqLogisticRegression(k, n, ctx=ctx, draws_per_step=D, learning_rate=1e-2)
        c.set_params(w, xb, zb)
        return c
    a = fresh()
    e1, e2 = a.loss_and_gradients(S, n, ap, y, seed=11), a.loss_and_gradients(S, n, ap, y, seed=11)
    assert e1[0] == e2[0]
    for g1, g2 in zip(e1[1:], e2[1:]):
        np.testing.assert_array_equal(g1, g2)
    assert a.loss_and_gradients(S, n, ap, y, seed=12)[0] != e1[0]  # (other draws)
    z0 = rng.normal(size=(5, D, S, n - 1)).astype(np.float32)
    for kw_split, kw_whole in ((lambda lo, hi: dict(seed=21), dict(seed=21)), (lambda lo, hi: dict(z0=z0[lo:hi]), dict(z0=z0))):
        a, b = fresh(), fresh()
        ta = np.concatenate([a.fit_steps_sample(S, n, ap, y, 2, **kw_split(0, 2)), a.fit_steps_sample(S, n, ap, y, 3, **kw_split(2, 5))])
        tb = b.fit_steps_sample(S, n, ap, y, 5, **kw_whole)
        np.testing.assert_array_equal(ta, tb)
        for pa, pb in zip(a.get_params(), b.get_params()):
            np.testing.assert_array_equal(pa, pb)
        assert not np.array_equal(a.get_params()[0], w)
    p1, p2 = a.predict_sample(S, n, ap, 4, seed=31), a.predict_sample(S, n, ap, 4, seed=31)
    np.testing.assert_array_equal(p1, p2)
    assert not np.array_equal(p1, a.predict_sample(S, n, ap, 4, seed=32))


@pytest.mark.parametrize("n,S,k,ndraws", [(150, 5, 3, 4), (1100, 5, 16, 2), (130, 1, 2, 3)])
def test_prediction_matches_restatement(P, ctx, n, S, k, ndraws):
    rng = np.random.default_rng(86)
    ap = _problem(P, ctx, S, n)
    z0 = rng.normal(size=(ndraws, S, n - 1)).astype(np.float32)
    lx = _draws(ap, z0)
    w, xb, zb = _params(rng, lx[0], n, k)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx)
    clf.set_params(w, xb, zb)
    probs = clf.predict_sample(S, n, ap, ndraws, z0=z0)
    ref = T.predict(w, xb, zb, lx)
    B = _B(lx, w)
    used = np.abs(probs - ref).max() / (2 * B)
    print("MARGIN predict n=%d S=%d k=%d draws=%d used %.3g" % (n, S, k, ndraws, used))
    assert probs.shape == (S, k) and used <= 1.0
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, rtol=0, atol=1e-6)
    one = clf.eval_sample(S, n, ap, z0=z0[0])
    assert np.abs(one - T.predict(w, xb, zb, lx[:1])).max() <= 2 * B


_PLANTED = {}


def _planted():
    """the construction of test_classify_recovers_the_classes_of_held_out_samples (tests/test_gpu_regression.py): n = 400, one shared
    tree, 30 planted effects of +-3, 8 training and 4 held-out samples of two classes, mu from the inverse transform, sigma 0.05"""
    if not _PLANTED:
        rng = np.random.default_rng(35)
        S, St, n = 8, 4, 400
        tree = random_tree(n, rng)
        to = O.PTT(*tree)
        base = rng.normal(0, 1.0, size=n)
        effect = np.zeros(n)
        effect[rng.choice(n, 30, replace=False)] = rng.choice([-3.0, 3.0], size=30)
        cls = np.array([0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0])
        mus, xs = [], []
        for s_ in range(S + St):
            logx = base + cls[s_] * effect + rng.normal(0, 0.05, size=n)
            x = np.exp(logx - logx.max())
            x /= x.sum()
            yy = np.clip(to.inverse_transform(x.astype(np.float32))[0], 1e-6, 1 - 1e-6)
            mus.append(np.log(yy) - np.log1p(-yy))
            xs.append(np.log(x))
        _PLANTED.update(S=S, St=St, n=n, tree=tree, cls=cls, mu=np.array(mus, np.float32), x_all=np.array(xs, np.float32))
    return _PLANTED


def test_end_to_end_recovers_the_classes_of_held_out_samples(P, ctx):
    """A float64 NumPy run of this model on this construction (draws modelled as log expression + N(0, 0.05)) goes from 5.545 to
    0.02-0.04 with the true class at 0.9987 or above, so the thresholds leave wide room."""
    c = _planted()
    S, St, n, cls, mu, x_all, k = c["S"], c["St"], c["n"], c["cls"], c["mu"], c["x_all"], 2
    li, ri, fi = O.make_inverse_ptt_params(*c["tree"])

    def vars_of(rows):
        m = len(rows)
        return dict(efflen=np.full((m, n), 1000.0, np.float32), la_mu=mu[rows], la_sigma=np.full((m, n - 1), 0.05, np.float32),
                    la_alpha=np.zeros((m, n - 1), np.float32), left_index=li[None], right_index=ri[None], leaf_index=fi[None])
    train, test = np.arange(S), np.arange(S, S + St)
    y = np.eye(k, dtype=np.float32)[cls[:S]]
    ap_train, ap_test = P.RNASeqApproxLikelihood(vars_of(train), ctx=ctx), P.RNASeqApproxLikelihood(vars_of(test), ctx=ctx)
    for point in (False, True):
        clf = P.RNASeqLogisticRegression(k, n, ctx=ctx, learning_rate=1e-3)
        if point:
            w, trace = clf.fit(x_all[train], y, 300, return_trace=True)
            probs = clf.predict(x_all[test])
        else:
            w, trace = clf.fit_sample(S, n, {"approx": ap_train}, y, 300, seed=5, return_trace=True)
            probs = clf.predict_sample(St, n, {"approx": ap_test}, 20, seed=9)
        print("end to end point=%s: loss %.4g -> %.4g, min p(true) %.5f" % (point, trace[0], trace[-50:].mean(),
                                                                           probs[np.arange(St), cls[test]].min()))
        assert w.shape == (n, k) and np.all(np.isfinite(trace))
        assert trace[-50:].mean() < 0.1 * trace[0]
        assert probs[np.arange(St), cls[test]].min() > 0.9, probs


@pytest.mark.parametrize("mode", ["likelihood", "point-estimates"])
def test_command_line_writes_the_three_files(P, tmp_path, mode):
    """python -m polee_amd.classify on the same construction, from prepared-sample files (or their TPM CSVs) and two experiment
    files: y-predicted.csv, y-true.csv and w.csv in the formats of models/classify.jl"""
    import json
    from polee_amd import classify, h5io
    c = _planted()
    S, St, n, cls = c["S"], c["St"], c["n"], c["cls"]
    names = ["sample%d" % i for i in range(S + St)]
    tissue = ["liver", "brain"]  # (class 0 = liver sorts after class 1 = brain)
    samples = []
    for i, name in enumerate(names):
        fn = str(tmp_path / (name + ".h5"))
        h5io.write_approximation(fn, 1000000, n, np.full(n, 1000.0, np.float32),
                                 dict(mu=c["mu"][i], omega=np.full(n - 1, np.log(0.05), np.float32), alpha=np.zeros(n - 1, np.float32),
                                      node_parent_idxs=c["tree"][0], node_js=c["tree"][1]))
        csv = str(tmp_path / (name + ".csv"))
        tpm = 1e6 * np.exp(c["x_all"][i].astype(np.float64))
        tpm[3] = 0.0  # (a zero TPM: the pseudocount keeps its log finite)
        with open(csv, "w") as f:
            f.write("transcript_id,tpm\n" + "".join("t%d,%r\n" % (j + 1, float(v)) for j, v in enumerate(tpm)))
        samples.append({"name": name, "file": fn, "factors": {"tissue": tissue[cls[i]]}, "point-estimates": {"tpm": csv}})
    (tmp_path / "train.yml").write_text(json.dumps({"samples": samples[:S]}))
    (tmp_path / "test.yml").write_text(json.dumps({"samples": samples[S:]}))
    (tmp_path / "ids.txt").write_text("".join("t%d\n" % (j + 1) for j in range(n)))
    out = [str(tmp_path / f) for f in ("p.csv", "t.csv", "w.csv")]
    argv = [str(tmp_path / "train.yml"), str(tmp_path / "test.yml"), "tissue", "--output-predictions", out[0], "--output-truth", out[1],
            "--output-w", out[2], "--num-steps", "300", "--learning-rate", "1e-3", "--testing-samples", "20", "--seed", "7"]
    if mode == "point-estimates":
        with pytest.raises(SystemExit) as ei:  # (log 0 without a pseudocount)
            classify.main(argv + ["--point-estimates", "tpm", "--transcript-ids", str(tmp_path / "ids.txt")])
        assert "--pseudocount" in str(ei.value.code)
        argv += ["--point-estimates", "tpm", "--transcript-ids", str(tmp_path / "ids.txt"), "--pseudocount", "1"]
    assert classify.main(argv) == 0
    truth = open(out[1]).read().splitlines()
    assert truth[0] == "brain,liver"
    assert truth[1:] == ["1.0,0.0" if tissue[cc] == "brain" else "0.0,1.0" for cc in cls[S:]]
    pred = open(out[0]).read().splitlines()
    assert pred[0] == "brain,liver" and len(pred) == St + 1
    probs = np.array([[float(v) for v in row.split(",")] for row in pred[1:]])
    want = np.array([0 if tissue[cc] == "brain" else 1 for cc in cls[S:]])
    assert probs[np.arange(St), want].min() > 0.9, probs
    w = np.loadtxt(out[2], delimiter="\t")
    assert w.shape == (n, 2) and np.isfinite(w).all() and np.abs(w).max() > 0  # (w starts at zero: training moved it)


def test_fit_keeps_the_options_of_the_constructor(P, ctx):
    """fit_sample / fit change draws_per_step / loss_scale only when the caller passes them"""
    rng = np.random.default_rng(87)
    n, S, k = 150, 5, 3
    ap = _problem(P, ctx, S, n)
    y = _labels(rng, S, k)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx, draws_per_step=2, loss_scale=0.7)
    _, trace = clf.fit_sample(S, n, ap, y, 1, seed=3, return_trace=True)
    assert clf.opts.draws_per_step == 2 and abs(trace[0] - 0.7 * S * np.log(k)) <= 1e-6 * S * np.log(k)
    clf.set_params(*(np.zeros_like(a) for a in clf.get_params()))
    _, trace = clf.fit(np.log(ap.sample(seed=4)), y, 1, return_trace=True)
    assert clf.opts.loss_scale == np.float32(0.7) and abs(trace[0] - 0.7 * S * np.log(k)) <= 1e-6 * S * np.log(k)
    clf.fit_sample(S, n, ap, y, 1, samples_per_iter=3)
    clf.fit(np.log(ap.sample(seed=4)), y, 1, loss_scale=1.0)
    assert clf.opts.draws_per_step == 3 and clf.opts.loss_scale == 1.0
    assert clf.loss_and_gradients(S, n, ap, y, seed=5)[1] is not None


def test_errors(P, ctx):
    n, S, k = 130, 1, 2
    ap = _problem(P, ctx, S, n)
    for bad in (1, 17):
        with pytest.raises(P.PoleeError) as ei:
            P.RNASeqLogisticRegression(bad, n, ctx=ctx)
        assert ei.value.status == 5 and "classes" in str(ei.value)
    clf = P.RNASeqLogisticRegression(k, n, ctx=ctx)
    for rows in ([[0.5, 0.5]], [[1.0, 1.0]], [[0.0, 0.0]], [[2.0, -1.0]]):
        with pytest.raises(P.PoleeError) as ei:
            clf.loss_and_gradients(S, n, ap, np.array(rows, np.float32))
        assert ei.value.status == 1 and "one-hot" in str(ei.value)
    other = P.RNASeqLogisticRegression(k, 150, ctx=ctx)
    with pytest.raises(P.PoleeError) as ei:  # (past the wrapper's own check: the library refuses an approximation of another n)
        P._lib.check(P.lib().polee_classify_init_bias(other._h, ap._h, None, C.c_uint64(0)), ctx._h)
    assert ei.value.status == 1 and "n = 130" in str(ei.value)
    x = np.zeros((2, n), np.float32)
    x[1, 7] = -np.inf
    with pytest.raises(P.NonFiniteError) as ei:
        clf.fit(x, np.eye(2, dtype=np.float32), 1)
    assert ei.value.status == 4 and "pseudocount" in str(ei.value)
    assert clf.loss_and_gradients(S, n, ap, np.array([[0.0, 1.0]], np.float32))[0] > 0  # (the handle still works)

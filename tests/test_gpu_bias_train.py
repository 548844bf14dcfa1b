"""The bias model trainer on the GPU (polee_amd/csrc/bias_train.hip) against its host twin and the NumPy
restatement of src/bias.jl (tests/bias_train_restatement.py): examples, orders, tables, GC bins and accuracy bit for bit, the loss
trace to the ulp error of log; one scored round from forced states that reach every table size (orders 0 .. 6, the LDS and the
global counting kernel); the background drawn on the device; and the trained model fed to build_likelihood_matrix."""
import numpy as np
import pytest

import bias_train_restatement as R
from oracle import xbuild as OX
from polee_amd import bias as B
from polee_amd import xbuild as XB
from tools import synth_aln

pytestmark = pytest.mark.gpu
MODEL_KEYS = ("orders_left", "orders_right", "ps_left", "ps_right", "gc_bins")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


@pytest.fixture(scope="module")
def ctx():
    import polee_amd as P
    return P.Context(0)


def _train(examples, ctx=None, host=False):
    left, right, gc, n_fg = examples
    with B.examples_trainer(left, right, gc, n_fg, host=host, ctx=ctx) as bt:
        ex = bt.examples(positions=False)
        m = bt.run().model()
    return ex, m


@pytest.mark.parametrize("case", ["planted", "2x33", "2x64"])
def test_device_trainer_matches_the_host_twin(ctx, case):
    """6002 examples (no multiple of 64 or 256), and 2 x 33 / 2 x 64 (a partial and an exact wave)"""
    if case == "planted":
        examples, ref = R.planted_reference()
        assert ref["gap"] >= 1e-6, ref["gap"]  # a condition on the input, not a tolerance
    else:
        examples = R.small_examples(int(case[2:]))
        ref = R.train(*examples)
        assert ref["gap"] >= 1e-6, ref["gap"]
    exh, h = _train(examples, host=True)
    exd, d = _train(examples, ctx=ctx)
    exd2, d2 = _train(examples, ctx=ctx)
    for key in ("left", "right", "frag_gc"):
        np.testing.assert_array_equal(exd[key], exh[key])
    for key in MODEL_KEYS:
        np.testing.assert_array_equal(np.asarray(d[key]).view(np.uint32), np.asarray(h[key]).view(np.uint32), err_msg=key)
        np.testing.assert_array_equal(np.asarray(d2[key]).view(np.uint32), np.asarray(d[key]).view(np.uint32), err_msg=key)
    assert d["accuracy"] == h["accuracy"] == ref["accuracy"] and d2["accuracy"] == d["accuracy"]
    worst = 0.0
    for side in ("left", "right"):
        key = "loss_trace_" + side
        assert len(d[key]) == len(h[key]) == len(ref[side]["trace"])
        np.testing.assert_array_equal(d2[key].view(np.uint64), d[key].view(np.uint64))  # two device runs: bitwise, the trace included
        worst = max(worst, rel(d[key], h[key]), rel(d[key], ref[side]["trace"]))
        np.testing.assert_array_equal(d["orders_" + side], ref[side]["orders"])
        np.testing.assert_array_equal(bits(d["ps_" + side]), bits(ref[side]["ps"]))
    print("device against host and restatement, %s: largest relative deviation of the loss trace %.3g" % (case, worst))
    assert worst <= 1e-12, worst


def _state(**at):
    o = np.full(20, -1, np.int32)
    for k, v in at.items():
        o[int(k[1:])] = v
    return o


FORCED = {
    "order 5 -> 6 at position 3": _state(p2=5),
    "order 5 -> 6 at position 14, reading through base 20": _state(p13=5),
    "position 20 at order 0": _state(p19=0),
    "mixed": _state(p0=0, p1=1, p2=2, p3=3, p4=4, p5=5, p6=6, p13=6, p18=1, p19=0),
}


@pytest.mark.parametrize("name", list(FORCED))
@pytest.mark.parametrize("side", [0, 1])
def test_candidates_from_forced_states_match_the_restatement(ctx, name, side):
    """one scored round on 6002 examples: tables of orders 0 .. 6 (8 to 32768 counters), all 20 losses within 1e-12 relative"""
    (left, right, gc, n_fg), _ = R.planted_reference()
    orders = FORCED[name]
    seq = (left, right)[side]
    want, want0 = R.candidate_losses(seq, np.arange(len(gc)) < n_fg, orders)
    with B.examples_trainer(left, right, gc, n_fg, ctx=ctx) as bt:
        got, got0 = bt.candidates(side, orders)
    with B.examples_trainer(left, right, gc, n_fg, host=True) as bt:
        host, host0 = bt.candidates(side, orders)
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isposinf(got), ~fin)
    np.testing.assert_array_equal(np.isposinf(host), ~fin)
    if name.startswith("position 20"):
        assert not fin[19] and fin[:19].all()
    if name == "mixed":
        assert (~fin).tolist() == [j in (6, 13, 18, 19) for j in range(20)]
    worst = max(rel(got[fin], want[fin]), rel(host[fin], want[fin]), rel(got0, want0), rel(host0, want0))
    print("candidates %s side %d: largest relative deviation %.3g" % (name, side, worst))
    assert worst <= 1e-12, worst


def test_examples_from_fragments_and_the_drawn_background(ctx):
    ptr, tseq, t, p, f, good = R.edge_fragments()
    seed = 0xFEDCBA9876543210
    d = B.bias_training_examples(ptr, tseq, t, p, f, seed=seed, ctx=ctx)
    h = B.bias_training_examples(ptr, tseq, t, p, f, seed=seed, host=True)
    assert d["dropped"] == 3 and d["n_fg"] == good == d["n_bg"]
    tlen = np.diff(ptr)[t[:good]]
    np.testing.assert_array_equal(d["bg_tpos"], R.bg_tpos(seed, np.arange(good), tlen - f[:good] + 1))
    for key in ("left", "right", "bg_tpos"):
        np.testing.assert_array_equal(d[key], h[key])
    np.testing.assert_array_equal(d["frag_gc"].view(np.uint64), h["frag_gc"].view(np.uint64))
    lf, rf, gf = R.make_examples(ptr, tseq, t[:good], p[:good], f[:good], seed, 1)
    np.testing.assert_array_equal(d["left"][:good], R.pack(lf))
    np.testing.assert_array_equal(d["right"][:good], R.pack(rf))
    # and the model trained from them, device against host
    md = B.train_bias_model(ptr, tseq, t, p, f, seed=seed, ctx=ctx)
    mh = B.train_bias_model(ptr, tseq, t, p, f, seed=seed, host=True)
    for key in MODEL_KEYS:
        np.testing.assert_array_equal(np.asarray(md[key]).view(np.uint32), np.asarray(mh[key]).view(np.uint32), err_msg=key)
    assert md["accuracy"] == mh["accuracy"]


def test_trained_model_through_build_likelihood_matrix(ctx):
    """n = 200 transcripts, m = 15000 fragments: the model trained on the device (tables of ps_ctx = 4096) goes into
    build_likelihood_matrix(bias=...); compared with oracle.xbuild under the same model as test_device_biased_model_matches_oracle
    (tests/test_xbuild.py) compares: bias vectors and effective lengths bit for bit, the same pattern, values to 1e-6."""
    n, m, seed = 200, 15000, 3
    d = synth_aln.make(n, m, seed=seed, p_single=0.2, p_noise=0.05)
    pmf0, _, _ = synth_aln.fraglen_model(180.0, 60.0)
    toy = synth_aln.make_bias_model(d["transcripts"], d["fragments"], pmf0, seed=seed + 10)
    ptr, tseq = toy["tseq_ptr"], toy["tseq"]
    # training fragments: positions kept more often when they start on C or G
    rng = np.random.default_rng(seed)
    tlen = np.diff(ptr)
    t = rng.choice(np.flatnonzero(tlen >= 120), 9000).astype(np.int32)
    fl = np.minimum(np.clip(np.rint(rng.normal(180, 60, len(t))), 20, 600), tlen[t]).astype(np.int32)
    pos = (1 + np.floor(rng.random(len(t)) * (tlen[t] - fl + 1))).astype(np.int64)
    first = tseq[ptr[t] + pos - 1]
    keep = rng.random(len(t)) < np.where((first == 1) | (first == 2), 0.9, 0.3)
    t, fl, pos = t[keep], fl[keep], pos[keep]
    model = B.train_bias_model(ptr, tseq, t, pos, fl, seed=seed, ctx=ctx)
    assert model["dropped"] == 0 and model["orders_left"][5] >= 0 and model["ps_left"].shape == (20, 4, 4096)
    flm = B.fragment_length_model(fl)
    pmf, cdf, med = flm["fraglen_pmf"], flm["fraglen_cdf"], flm["fraglen_median"]
    bias = dict(tseq_ptr=ptr, tseq=tseq, m1_reverse=toy["m1_reverse"], **model, **flm)
    Ts, Fs, Ms, keep_ = XB.pack(d["transcripts"], d["fragments"], pmf, cdf, med, 0.85, False)
    Bs, kb = XB.pack_bias(bias)
    o = OX.build_biased(Ts, Fs, Ms, Bs, n, int(ptr[-1]))
    g = XB.build_likelihood_matrix(d["transcripts"], d["fragments"], pmf, cdf, med, 0.85, False, ctx=ctx, bias=bias, return_bias=True)
    np.testing.assert_array_equal(g["right_bias"], o["right_bias"])
    np.testing.assert_array_equal(g["left_bias"], o["left_bias"])
    np.testing.assert_array_equal(g["effective_lengths"], o["effective_lengths"])
    assert g["m"] == o["m"] and g["nnz"] == o["nnz"] and g["m"] > 0.8 * m
    np.testing.assert_array_equal(g["row_fragment"], o["row_fragment"])
    np.testing.assert_array_equal(g["trowval"], o["trowval"])
    np.testing.assert_allclose(g["tnzval"], o["tnzval"], rtol=1e-6)
    assert len(np.unique(g["left_bias"])) >= 4  # the trained model does weigh positions (order 0 at the fragment's first base: four values)

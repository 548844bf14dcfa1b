"""The bias model trainer without a GPU: the host trainer (polee_amd/csrc/bias_train_host.cpp, `host=True`)
against the NumPy restatement of src/bias.jl (tests/bias_train_restatement.py) -- examples and background draws bit for bit, the
trained model bit for bit, the loss trace to the ulp error of log -- a hand-computed candidate, argument validation, the fragment
length model, the command line and the reader of the reference's dump files."""
import math
import os
import re

import numpy as np
import pytest

import bias_train_restatement as R
from conftest import ROOT
from polee_amd import _lib as L
from polee_amd import bias as B
from polee_amd import xbuild as XB

NEW_EXPORTS = ("polee_bias_train_create", "polee_bias_train_create_from_examples", "polee_bias_train_run", "polee_bias_train_get_model",
               "polee_bias_train_get_examples", "polee_bias_train_get_trace", "polee_bias_train_destroy", "polee_bias_train_candidates")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def test_exports_julia_wrappers_and_package_names():
    import polee_amd as P
    lib = L.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polee_hip.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "PoleeHIP.jl")).read()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert (":" + name) in jl, name
    for name in ("train_bias_model", "train_bias_model_from_examples", "fragment_length_model", "read_reference_dump"):
        assert getattr(P, name) is getattr(B, name)


def test_hand_computed_candidate_on_32_examples():
    """16 + 16 examples, every base A except position 1: foreground 16 A, background 4 of each base.  The candidate
    (position 1, order 0) has counts fg [16, 0, 0, 0], bg [4, 4, 4, 4], tables (1 + count) / 20, and the loss below; every other
    position's candidate has equal tables in both classes, p = 1/2, and only pays its 4 log(32)."""
    left = np.zeros((32, 20), np.uint8)
    left[16:, 0] = [0, 1, 2, 3] * 4
    right, gc = np.zeros((32, 20), np.uint8), np.full(32, 0.5)
    ps_fg = np.array([17, 1, 1, 1], f32) / f32(20)
    ps_bg = np.array([5, 5, 5, 5], f32) / f32(20)
    ll = 0.0
    for e in range(32):
        nt = left[e, 0]
        p = f32(ps_fg[nt] / f32(ps_fg[nt] + ps_bg[nt]))
        ll += math.log(float(p if e < 16 else f32(f32(1) - p)))
    loss_hand = -(2 * ll - 4 * math.log(32))
    null = -(2 * 32 * math.log(0.5))
    with B.examples_trainer(left, right, gc, 16, host=True) as bt:
        losses, loss0 = bt.candidates(0, np.full(20, -1, np.int32))
        m = bt.run().model()
    assert abs(loss0 - null) <= 1e-12 * null
    assert abs(losses[0] - loss_hand) <= 1e-12 * loss_hand
    np.testing.assert_allclose(losses[1:], null + 4 * math.log(32), rtol=1e-12)
    assert loss_hand < null
    # the trained model: that one round, and the table row fg / bg of the hand counts
    assert m["orders_left"].tolist() == [0] + [-1] * 19 and m["orders_right"].tolist() == [-1] * 20
    np.testing.assert_array_equal(bits(m["ps_left"][0, :, 0]), bits(ps_fg / ps_bg))
    assert (m["ps_left"][0, :, 1:] == 1).all() and (m["ps_left"][1:] == 1).all() and (m["ps_right"] == 1).all()
    assert len(m["loss_trace_left"]) == 2 and abs(m["loss_trace_left"][1] - loss_hand) <= 1e-12 * loss_hand
    assert (m["gc_bins"] == 1).all()  # every frag_gc equal: one occupied bin, 17/31 over 17/31


def test_examples_and_background_draws_match_the_restatement_bitwise():
    ptr, tseq, t, p, f, good = R.edge_fragments()
    assert (tseq == 4).any() and good >= 100
    seed = 0x1234567890ABCDEF
    ex = B.bias_training_examples(ptr, tseq, t, p, f, seed=seed, host=True)
    assert ex["dropped"] == 3 and ex["n_fg"] == good and ex["n_bg"] == good
    t, p, f = t[:good], p[:good], f[:good]
    tlen = np.diff(ptr)[t]
    bg = R.bg_tpos(seed, np.arange(good), tlen - f + 1)
    np.testing.assert_array_equal(ex["bg_tpos"], bg)
    assert (bg >= 1).all() and (bg + f - 1 <= tlen).all() and len(set((bg - 1).tolist())) > 10
    lf, rf, gf = R.make_examples(ptr, tseq, t, p, f, seed, 1)
    lb, rb, gb = R.make_examples(ptr, tseq, t, bg, f, seed, 0)
    np.testing.assert_array_equal(ex["left"], np.concatenate([R.pack(lf), R.pack(lb)]))
    np.testing.assert_array_equal(ex["right"], np.concatenate([R.pack(rf), R.pack(rb)]))
    np.testing.assert_array_equal(ex["frag_gc"].view(np.uint64), np.concatenate([gf, gb]).view(np.uint64))
    # fraglen 20 at positions 1 .. : the windows overlap in 10 bases (offsets 10 .. 19 of the padded fragment)
    k = int(np.flatnonzero(f == 20)[0])
    np.testing.assert_array_equal(lf[k][10:], rf[k][:10])
    # a given background equal to the drawn one gives the same examples
    ex2 = B.bias_training_examples(ptr, tseq, t, p, f, background=(t, bg, f), seed=seed, host=True)
    for key in ("left", "right", "frag_gc", "bg_tpos"):
        np.testing.assert_array_equal(ex2[key], ex[key])
    # another seed moves the pads and the draws
    ex3 = B.bias_training_examples(ptr, tseq, t, p, f, seed=seed + 1, host=True)
    assert (ex3["bg_tpos"] != ex["bg_tpos"]).any() and (ex3["left"][:good] != ex["left"][:good]).any()


def check_against_restatement(m, ref, tol=1e-12):
    """orders equal; ps bitwise where the model reads and 1.0 elsewhere; gc_bins bitwise; accuracy equal; traces within tol.
    -> the largest relative deviation of the traces"""
    worst = 0.0
    for side in ("left", "right"):
        o = ref[side]["orders"]
        np.testing.assert_array_equal(m["orders_" + side], o)
        ps = m["ps_" + side]
        np.testing.assert_array_equal(bits(ps), bits(ref[side]["ps"]))
        for j in range(20):
            used = 0 if o[j] < 0 else 4 ** o[j]
            assert (ps[j, :, used:] == 1.0).all()
        assert len(m["loss_trace_" + side]) == len(ref[side]["trace"])
        worst = max(worst, rel(m["loss_trace_" + side], ref[side]["trace"]))
    np.testing.assert_array_equal(bits(m["gc_bins"]), bits(ref["gc_bins"]))
    assert m["accuracy"] == ref["accuracy"]
    assert worst <= tol, worst
    return worst


def test_host_trainer_matches_the_restatement_on_the_planted_case():
    (left, right, gc, n_fg), ref = R.planted_reference()
    assert ref["gap"] >= 1e-6, ref["gap"]  # a condition on the input: no decision of the search is within reach of log's ulps
    assert len(gc) == 6002 and len(ref["left"]["trace"]) == 8
    assert [int(ref["left"]["orders"][j]) for j in (2, 5, 18, 19)] == [0, 2, 1, 0] and (ref["left"]["orders"] >= 0).sum() == 4
    m = B.train_bias_model_from_examples(left, right, gc, n_fg, host=True)
    worst = check_against_restatement(m, ref)
    print("host trainer against the restatement, planted case: largest relative deviation of the loss trace %.3g" % worst)
    assert 0.5 < m["accuracy"] <= 1.0


def test_argument_validation():
    ptr, tseq, t, p, f, good = R.edge_fragments()
    t, p, f = t[:good], p[:good], f[:good]
    with pytest.raises(L.PoleeError) as e:  # too few examples: 14 + 14
        B.bias_trainer(ptr, tseq, t[:14], p[:14], f[:14], host=True)
    assert e.value.status == 1 and "30" in str(e.value)
    h = L.C.c_void_p()
    opts = L.BiasTrainOpts(0, 1, 0)

    def create(t_, p_, f_):
        t_, p_, f_ = L.arr(t_, np.int32), L.arr(p_, np.int64), L.arr(f_, np.int32)
        return L.lib().polee_bias_train_create(None, len(ptr) - 1, L.ptr(ptr, L.i64p), L.ptr(tseq, L.u8p), len(t_), L.ptr(t_, L.i32p),
                                               L.ptr(p_, L.i64p), L.ptr(f_, L.i32p), 0, None, None, None, L.C.byref(opts), L.C.byref(h))
    f2 = f.copy(); f2[7] = 19
    assert create(t, p, f2) == 1 and b"fraglen 19" in L.lib().polee_last_error(None)
    p2 = p.copy(); p2[7] = 0
    assert create(t, p2, f) == 1
    p2[7] = np.diff(ptr)[t[7]] - f[7] + 2
    assert create(t, p2, f) == 1 and h.value is None
    t2 = t.copy(); t2[0] = len(ptr) - 1
    assert create(t2, p, f) == 1
    # 2^24 examples: unsupported (checked before anything is read)
    z = np.zeros((1, 20), np.uint8)
    assert L.lib().polee_bias_train_create_from_examples(None, 1 << 23, 1 << 23, L.ptr(z, L.u8p), L.ptr(z, L.u8p),
                                                         L.ptr(np.zeros(1), L.f64p), L.C.byref(opts), L.C.byref(h)) == 5
    # the device trainer needs a context
    dev = L.BiasTrainOpts(0, 0, 0)
    assert L.lib().polee_bias_train_create_from_examples(None, 16, 16, L.ptr(np.zeros((32, 20), np.uint8), L.u8p),
                                                         L.ptr(np.zeros((32, 20), np.uint8), L.u8p), L.ptr(np.zeros(32), L.f64p),
                                                         L.C.byref(dev), L.C.byref(h)) == 1
    with B.examples_trainer(np.zeros((32, 20), np.uint8), np.zeros((32, 20), np.uint8), np.zeros(32), 16, host=True) as bt:
        with pytest.raises(L.PoleeError):  # not trained yet
            bt.model()
        with pytest.raises(L.PoleeError):  # order 1 at position 20 reads past the end
            bt.candidates(0, [-1] * 19 + [1])
        with pytest.raises(L.PoleeError):  # made from examples: no positions
            bt.examples(positions=True)


def test_fragment_length_model_on_a_hand_case():
    fl = np.concatenate([np.full(500, 200), np.full(300, 180), np.full(300, 220), np.full(5, 2000), np.full(7, 2001)])
    m = B.fragment_length_model(fl)
    total = f32(2000 + 1105)  # pseudocount 1 each + the 1105 lengths <= 2000
    assert m["fraglen_pmf"].dtype == np.float32 and m["fraglen_pmf"][199] == f32(501) / total and m["fraglen_pmf"][0] == f32(1) / total
    assert m["fraglen_pmf"][1999] == f32(6) / total
    np.testing.assert_array_equal(m["fraglen_cdf"], np.cumsum(m["fraglen_pmf"], dtype=np.float32))
    assert m["fraglen_median"] == 453  # from 220 on, cdf[l] = (l + 1100) / 3105: the first l with cdf >= 1/2 is ceil(452.5)
    # descending, the tie between 180 and 220 keeps the shorter first, then 2000, then the pseudocount-only lengths in order
    assert m["high_prob_fraglens"][:6].tolist() == [200, 180, 220, 2000, 1, 2] and len(m["high_prob_fraglens"]) == 200
    # below MIN_FRAG_LEN_COUNT observations: the fallback normal (150, 50)
    fb = B.fragment_length_model(fl[:999])
    assert fb["high_prob_fraglens"][:3].tolist() == [150, 149, 151] and fb["fraglen_median"] == 150
    assert abs(float(fb["fraglen_cdf"][-1]) - 1) < 1e-5


def test_command_line_round_trip_and_pack_bias(tmp_path):
    ptr, tseq, t, p, f, good = R.edge_fragments()
    src, dst = str(tmp_path / "fragments.npz"), str(tmp_path / "bias-model.npz")
    np.savez(src, tseq_ptr=ptr, tseq=tseq, transcript=t, tpos=p, fraglen=f)
    assert B.main([src, "-o", dst, "--seed", "5", "--host"]) == 0
    z = np.load(dst)
    direct = B.train_bias_model(ptr, tseq, t, p, f, seed=5, host=True)
    assert int(z["dropped"]) == 3 == direct["dropped"]
    for key in ("orders_left", "orders_right", "ps_left", "ps_right", "gc_bins", "loss_trace_left", "loss_trace_right"):
        np.testing.assert_array_equal(z[key], direct[key])
    assert set(direct) == {"orders_left", "orders_right", "ps_left", "ps_right", "gc_bins", "accuracy", "loss_trace_left",
                           "loss_trace_right", "dropped"}
    bias = {k: z[k] for k in z.files}
    Bs, keep = XB.pack_bias(bias)
    assert Bs.seqbias_len == 20 and Bs.ps_ctx == 4096 and Bs.gc_nbins == 100 and Bs.num_fraglens == 200 and not Bs.pos_terms
    np.testing.assert_array_equal(z["high_prob_fraglens"], B.fragment_length_model(f)["high_prob_fraglens"])
    np.testing.assert_array_equal(z["tseq"], tseq)


def test_reference_dump_reader(tmp_path):
    (left, right, gc, n_fg), _ = R.planted_reference()
    pick = np.concatenate([np.arange(40), n_fg + np.arange(35)])
    letters = np.array(list("ACGT"))
    paths = []
    for name, rows in (("bias-foreground.csv", pick[:40]), ("bias-background.csv", pick[40:])):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w") as out:
            for k, e in enumerate(rows):
                ls = "".join(letters[left[e]])
                if k == 0 and name == "bias-foreground.csv":
                    ls = "N" + ls[1:]
                # left_seq,right_seq,frag_gc,tpdist,fpdist,tlen,flen, then 4 x 4 frequencies (fragmodel.jl:306-339)
                out.write(",".join([ls, "".join(letters[right[e]]), repr(float(gc[e])), "10", "300", "1000", "250"] + ["0.25"] * 16) + "\n")
    l, r, g, nf = B.read_reference_dump(*paths)
    assert nf == 40 and l.shape == (75, 20) and l[0, 0] == 4
    np.testing.assert_array_equal(l[1:], left[pick][1:])
    np.testing.assert_array_equal(r, right[pick])
    np.testing.assert_array_equal(g, gc[pick])
    dst = str(tmp_path / "m.npz")
    assert B.main(["--reference-dump", paths[0], paths[1], "-o", dst, "--host"]) == 0
    l0 = left[pick].copy()
    l0[0, 0] = 0  # N -> A
    ref = R.train(l0, right[pick], gc[pick], 40)
    z = np.load(dst)
    np.testing.assert_array_equal(z["orders_left"], ref["left"]["orders"])
    np.testing.assert_array_equal(bits(z["gc_bins"]), bits(ref["gc_bins"]))
    assert float(z["accuracy"]) == ref["accuracy"]
    with open(paths[0], "a") as out:
        out.write("ACGT,ACGT,0.5\n")
    with pytest.raises(ValueError):
        B.read_reference_dump(*paths)

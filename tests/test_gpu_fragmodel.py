"""The fragment model from alignment pairs on the GPU (polee_fragmodel_estimate, polee_read_assign in polee_amd/csrc/xbuild.hip; DESIGN.md
section 3.18) against the plain Python restatement (tests/fragmodel_restatement.py): integers, compared exactly."""
import numpy as np
import pytest

import fragmodel_restatement as FR
from polee_amd import fragmodel as FM
from polee_amd import xbuild as XB
from tools import synth_aln

pytestmark = pytest.mark.gpu
FIELDS = ("transcript", "tpos", "fraglen", "flags")


@pytest.fixture(scope="module")
def ctx():
    import polee_amd as P
    return P.Context(0)


@pytest.fixture(scope="module")
def data():
    """60 transcripts on both strands, 3000 fragments, a tenth of them single-end; sequences and m1_reverse (seeded, both ways)"""
    d = synth_aln.make(60, 3000, seed=5)
    T, F = d["transcripts"], XB.order_mates(d["fragments"])
    toy = synth_aln.make_bias_model(T, F, synth_aln.fraglen_model()[0], seed=15)
    single = np.asarray(F["m2_left"]) == 0
    assert set(np.unique(T["strand"]).tolist()) == {-1, 1} and single.sum() > 100
    assert 0 < toy["m1_reverse"][single].sum() < single.sum()
    return dict(T=T, F=F, tseq_ptr=toy["tseq_ptr"], tseq=toy["tseq"], m1_reverse=toy["m1_reverse"], true_transcript=d["true_transcript"])


def _estimate_equals(ctx, T, F, want):
    got = FM.fragmodel_counts(T, F, ctx)
    print("counts", got["counts"].tolist(), "restated", want["counts"].tolist())
    assert got["counts"].tolist() == want["counts"].tolist()
    np.testing.assert_array_equal(got["hist"], want["hist"])
    np.testing.assert_array_equal(got["min_fraglen"], want["min_fraglen"])
    again = FM.fragmodel_counts(T, F, ctx)
    assert all(np.array_equal(got[k], again[k]) for k in got)
    return got


@pytest.mark.parametrize("m", [3000, 400, 37])
def test_estimate_matches_the_restatement(ctx, data, m):
    """3000 fragments: 11 full workgroups and a tail of 184; 400: below the 1000 lengths of the counted pmf (the fallback); 37: less
    than a wave"""
    if m == 3000:
        T, F = data["T"], data["F"]
    else:
        d = synth_aln.make(60, m, seed=5)
        T, F = d["transcripts"], XB.order_mates(d["fragments"])
    want = FR.estimate(T, F)
    got = _estimate_equals(ctx, T, F, want)
    assert got["counts"][1] + got["counts"][2] > 0 and (got["min_fraglen"] > 0).sum() == got["hist"].sum() + got["counts"][3]
    fm = FM.estimate_simplistic(T, F, ctx=ctx)
    ref = FM.simplistic_from_counts(want["counts"], want["hist"])
    assert fm["fraglen_median"] == ref["fraglen_median"] and fm["strand_specificity"] == ref["strand_specificity"]
    assert fm["fraglen_pmf"].tobytes() == ref["fraglen_pmf"].tobytes() and fm["fraglen_cdf"].tobytes() == ref["fraglen_cdf"].tobytes()
    assert (got["hist"].sum() < 1000) == (m != 3000)
    assert fm["counts"]["compatible_pairs"] == want["counts"][0]


def test_estimate_when_one_bin_takes_every_increment(ctx, data):
    """5000 copies of one paired fragment: every thread of 20 workgroups adds to the same LDS bin"""
    T, F = data["T"], data["F"]
    one = FR.estimate(T, F)["min_fraglen"]
    i = int(np.flatnonzero((one > 0) & (np.asarray(F["m2_left"]) > 0))[0])
    single = FR.estimate(T, FM.take_fragments(F, [i]))
    l = int(single["min_fraglen"][0])
    copies = FM.take_fragments(F, [i] * 5000)
    want = dict(counts=single["counts"] * 5000, hist=single["hist"] * 5000, min_fraglen=np.full(5000, l, np.int64))
    got = _estimate_equals(ctx, T, copies, want)
    assert got["hist"][l - 1] == 5000 and got["hist"].sum() == 5000


@pytest.fixture(scope="module")
def built(ctx, data):
    """X of the 3000 fragments on the device under the model estimated from them, and a seeded mixture"""
    T, F = data["T"], data["F"]
    fm = FM.estimate_simplistic(T, F, ctx=ctx)
    x = XB.build_likelihood_matrix(T, F, fm["fraglen_pmf"], fm["fraglen_cdf"], fm["fraglen_median"], fm["strand_specificity"], ctx=ctx,
                                   return_xbuild=True)
    xs = np.random.default_rng(21).dirichlet(np.ones(T["n"])).astype(np.float32)
    yield x, xs
    x["xbuild"].close()


def test_assign_matches_the_restatement_in_both_modes(ctx, data, built):
    T, F = data["T"], data["F"]
    x, xs = built
    assert x["m"] > 2500 and (np.diff(x["tcolptr"].astype(np.int64)) > 1).sum() > 1000
    draws = {}
    for assign, mode in (("draw", 0), ("reference", 1)):
        want = FR.assign(T, F, x, xs, data["m1_reverse"], 7, mode)
        got = FM.assign_reads(x["xbuild"], T, F, data["tseq_ptr"], xs, data["m1_reverse"], seed=7, assign=assign, ctx=ctx)
        for k in FIELDS:
            assert got[k].dtype == want[k].dtype
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (assign, k))
        again = FM.assign_reads(x["xbuild"], T, F, data["tseq_ptr"], xs, data["m1_reverse"], seed=7, assign=assign, ctx=ctx)
        other = FM.assign_reads(x["xbuild"], T, F, data["tseq_ptr"], xs, data["m1_reverse"], seed=8, assign=assign, ctx=ctx)
        assert all(np.array_equal(got[k], again[k]) for k in FIELDS)
        assert all(np.array_equal(got[k], other[k]) for k in FIELDS) == (mode == 1)
        draws[mode] = got
    # the inputs reach every branch: single-end rows with the lone mate either way, both strand outcomes, lengths that were guessed
    flags, rf = draws[0]["flags"], x["row_fragment"]
    lone = (flags & FR.FLAG_OBSERVED) == 0
    assert lone.sum() > 100 and 0 < data["m1_reverse"][rf[lone]].sum() < lone.sum()
    assert ((flags & FR.FLAG_STRAND_MATCH) != 0).sum() > 1000 and ((flags & FR.FLAG_STRAND_MISMATCH) != 0).sum() > 50
    assert (draws[0]["transcript"] != draws[1]["transcript"]).sum() > 100  # the draw is not the last entry
    last = x["trowval"].astype(np.int64)[x["tcolptr"].astype(np.int64)[1:] - 2] - 1
    np.testing.assert_array_equal(draws[1]["transcript"], last)
    # mode 1 needs neither xs nor a seed
    none = FM.assign_reads(x["xbuild"], T, F, data["tseq_ptr"], None, data["m1_reverse"], assign="reference", ctx=ctx)
    assert all(np.array_equal(none[k], draws[1][k]) for k in FIELDS)


def test_interval_of_overhanging_fragments(ctx):
    """The interval the kernel reports equals genomic_to_transcriptomic of the restatement where the nudge acts: fragments soft-clipped
    past an exon's end and single-end reads whose guessed length runs past either end of a transcript, on both strands."""
    T, F, rev, expected = FR.overhang_case()
    pmf = np.full(2000, 1.0 / 2000.0, np.float32)
    x = XB.build_likelihood_matrix(T, F, pmf, np.cumsum(pmf, dtype=np.float32), 1000, 0.5, ctx=ctx, return_xbuild=True)
    try:
        assert (x["m"], x["nnz"]) == (5, 10) and x["row_fragment"].tolist() == [0, 1, 2, 3, 4]
        tseq_ptr = np.array([0, 200, 400], np.int64)
        for j, xs in ((0, [1.0, 0.0]), (1, [0.0, 1.0])):
            got = FM.assign_reads(x["xbuild"], T, F, tseq_ptr, np.array(xs, np.float32), rev, seed=3, assign="draw", ctx=ctx)
            want = FR.assign(T, F, x, np.array(xs, np.float32), rev, 3, 0)
            for k in FIELDS:
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
            assert got["transcript"].tolist() == [j] * 5
            assert list(zip(got["tpos"].tolist(), got["fraglen"].tolist())) == [expected[(i, j)] for i in range(5)]
        last = FM.assign_reads(x["xbuild"], T, F, tseq_ptr, None, rev, assign="reference", ctx=ctx)
        assert last["transcript"].tolist() == [1] * 5 and last["flags"].tolist() == [1 | 4, 1 | 4, 4, 2, 1 | 4]
        # no guess for the length: single-end fragments get the empty interval and no strand bit
        none = FM.assign_reads(x["xbuild"], T, F, tseq_ptr, None, rev, assign="reference", fallback_fraglen=0, ctx=ctx)
        assert none["fraglen"].tolist() == [95, 94, 0, 0, 80] and none["tpos"].tolist() == [11, 1, 0, 0, 101]
        assert none["flags"].tolist() == [1 | 4, 1 | 4, 0, 0, 1 | 4]
    finally:
        x["xbuild"].close()


@pytest.mark.parametrize("mixture", ["optimize", "em"])
def test_train_fragment_model_end_to_end(ctx, data, mixture):
    T, F = data["T"], data["F"]
    N, seed = 1500, 2
    out = FM.train_fragment_model(T, F, data["tseq_ptr"], data["tseq"], data["m1_reverse"], num_training_reads=N, seed=seed,
                                  mixture=mixture, ctx=ctx)
    sub, idx = FM.subsample_fragments(F, N, seed)
    diag = out["diagnostics"]
    np.testing.assert_array_equal(diag["indices"], idx)
    fm = FM.estimate_simplistic(T, sub, ctx=ctx)
    for k in ("fraglen_median", "strand_specificity", "alt_frag_model"):
        assert out["fragmodel"][k] == fm[k]
    for k in ("fraglen_pmf", "fraglen_cdf"):
        assert out["fragmodel"][k].tobytes() == fm[k].tobytes()
    # the assignment of the run equals the restatement's on the same X and the run's mixture, and so does the share of true transcripts
    x = XB.build_likelihood_matrix(T, sub, fm["fraglen_pmf"], fm["fraglen_cdf"], fm["fraglen_median"], fm["strand_specificity"], ctx=ctx)
    np.testing.assert_array_equal(x["row_fragment"], diag["row_fragment"])
    xs = diag["xs"]
    assert xs.dtype == np.float32 and abs(float(xs.sum()) - 1.0) < 1e-3
    want = FR.assign(T, sub, x, xs, data["m1_reverse"][idx], seed, 0)
    for k in FIELDS:
        np.testing.assert_array_equal(diag[k], want[k], err_msg=k)
    truth = data["true_transcript"][idx][x["row_fragment"]]
    frac, frac_restated = float((diag["transcript"] == truth).mean()), float((want["transcript"] == truth).mean())
    print("mixture %s: %d rows, share assigned to the true transcript %.6f (restated %.6f)" % (mixture, x["m"], frac, frac_restated))
    assert frac == frac_restated
    # the bias model is what build_likelihood_matrix takes, on the full fragments
    b = out["bias"]
    assert b is not None and 0.0 < b["accuracy"] <= 1.0 and b["m1_reverse"] is not None
    lm = FM.biased_from_assignment(data["tseq_ptr"], want)
    assert b["fraglen_median"] == lm["fraglen_median"] and b["strand_specificity"] == lm["strand_specificity"]
    np.testing.assert_array_equal(b["high_prob_fraglens"], lm["high_prob_fraglens"])
    full = XB.build_likelihood_matrix(T, F, b["fraglen_pmf"], b["fraglen_cdf"], b["fraglen_median"], b["strand_specificity"], ctx=ctx, bias=b)
    assert full["m"] > 0 and full["nnz"] >= full["m"] and np.isfinite(full["tnzval"]).all() and (full["tnzval"] > 0).all()
    assert np.isfinite(full["effective_lengths"]).all()


def test_train_fragment_model_without_bias(ctx, data):
    out = FM.train_fragment_model(data["T"], data["F"], data["tseq_ptr"], data["tseq"], data["m1_reverse"], no_bias=True, ctx=ctx)
    assert out["bias"] is None and len(out["diagnostics"]["indices"]) == 2545
    fm = FM.estimate_simplistic(data["T"], FM.subsample_fragments(data["F"])[0], ctx=ctx)
    assert out["fragmodel"]["fraglen_pmf"].tobytes() == fm["fraglen_pmf"].tobytes()
    assert out["fragmodel"]["strand_specificity"] == fm["strand_specificity"]
    with pytest.raises(ValueError):
        FM.train_fragment_model(data["T"], data["F"], data["tseq_ptr"], data["tseq"], assign="nearest", ctx=ctx)

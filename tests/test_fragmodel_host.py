"""Host checks (no GPU) of the fragment model from alignment pairs (polee_amd/fragmodel.py): the restatement's
fragmentlength against the existing oracle through a probe model, the estimate on a hand-made case, the from-histogram length model
against bias.fragment_length_model, the subsample, the draw, the command line and the exports."""
import ctypes as C
import math

import numpy as np
import pytest

import fragmodel_restatement as FR
from oracle import xbuild as OX
from polee_amd import bias as B
from polee_amd import fragmodel as FM
from polee_amd import xbuild as XB
from tools import synth_aln

NEW_SYMBOLS = ("polee_fragmodel_estimate", "polee_read_assign")


@pytest.fixture(scope="module")
def data():
    d = synth_aln.make(60, 3000, seed=5)
    return d["transcripts"], XB.order_mates(d["fragments"])


@pytest.fixture(scope="module")
def restated(data):
    return FR.estimate(*data)


def test_restated_fragmentlength_against_the_oracle_through_a_probe_model(data, restated):
    """Probe model: fraglen_pmf[l-1] = l, strand_specificity 0.5, efflen 1, no alt model: xb_oracle_condfragprob is 0.5 fraglen for a
    compatible paired fragment of length <= 2000.  Every entry the oracle keeps agrees with the restatement."""
    T, F = data
    n, m = T["n"], F["m"]
    pmf = np.arange(1, 2001, dtype=np.float32)
    Ts, Fs, Ms, keep = XB.pack(T, F, pmf, np.ones(2000, np.float32), 1, 0.5, False)
    out = OX.build(Ts, Fs, Ms, n)
    assert (out["m"], out["nnz"]) == (2851, 6597)
    L = OX.lib()
    rows = np.repeat(np.arange(out["m"]), np.diff(out["tcolptr"].astype(np.int64)))
    frag, tj = out["row_fragment"][rows], out["trowval"].astype(np.int64) - 1
    mine = {(i, j): fl for i, j, fl in restated["pairs"]}
    paired = np.asarray(F["m2_left"]) > 0
    lens = {}
    for i, j in zip(frag.tolist(), tj.tolist()):
        assert (i, j) in mine  # compatible in the restatement too
        if not paired[i]:
            assert mine[(i, j)] == 0
            continue
        p = L.xb_oracle_condfragprob(C.byref(Ts), C.byref(Fs), C.byref(Ms), C.c_int32(j), C.c_int64(i), C.c_float(1.0))
        assert 2.0 * p == mine[(i, j)], (i, j, p, mine[(i, j)])
        lens.setdefault(i, []).append(mine[(i, j)])
    # every compatible pair of the restatement with a visible probability is an entry of the oracle's
    assert {k for k, fl in mine.items() if fl <= 2000} == set(zip(frag.tolist(), tj.tolist()))
    mins = np.array([min(v) for v in lens.values()])
    assert (len(lens), mins.min(), mins.max()) == (2581, 72, 334)
    assert sum(1 for v in lens.values() if min(v) != max(v)) == 45  # the transcripts disagree on the length: the minimum matters
    got = restated["min_fraglen"]
    assert all(got[i] == min(v) for i, v in lens.items()) and (got > 0).sum() == 2581


def _hand_case():
    """one two-exon transcript (+, exons 101..200 and 301..400); fragments: three paired on +, one paired on -, one of strand 0
    (STRAND_BOTH), one single-end, one incompatible (a match across the intron), one on another sequence"""
    T = dict(n=1, seq=np.array([0], np.int32), strand=np.array([1], np.int8), exon_ptr=np.array([0, 2], np.int64),
             exon_first=np.array([101, 301], np.int64), exon_last=np.array([200, 400], np.int64))
    #        seq strand m1_left m1_right m2_left m2_right cigar1            cigar2
    frags = [(0, 1, 111, 160, 331, 380, [], []),                      # spans the intron: 380 - 111 + 1 - 100 = 170
             (0, 1, 111, 160, 141, 190, [], []),                      # inside exon 1: 80
             (0, 1, 151, 350, 331, 380, [(0, 50), (3, 100), (0, 50)], []),  # first mate spliced: 380 - 151 + 1 - 100 = 130
             (0, -1, 311, 360, 341, 390, [], []),                     # the other strand: 80
             (0, 0, 121, 170, 151, 200, [], []),                      # STRAND_BOTH: 80, neither match nor mismatch
             (0, 1, 121, 170, 0, 0, [], []),                          # single-end: compatible, no length
             (0, 1, 151, 350, 0, 0, [], []),                          # one match across the intron: incompatible
             (1, 1, 111, 160, 141, 190, [], [])]                      # no transcript on sequence 1
    return T, FR.make_fragments(frags)


def test_estimate_on_a_hand_made_case():
    T, F = _hand_case()
    e = FR.estimate(T, F)
    assert e["min_fraglen"].tolist() == [170, 80, 130, 80, 80, 0, 0, 0]
    assert e["counts"].tolist() == [6, 4, 1, 0]  # six compatible pairs; + + four times (the single-end one too), - once, strand 0 neither
    want = np.zeros(2000, np.int64)
    want[[169, 129]] = 1
    want[79] = 3
    assert (e["hist"] == want).all()
    fm = FM.simplistic_from_counts(e["counts"], e["hist"])
    assert fm["strand_specificity"] == float(np.float32(0.8))
    with pytest.raises(ValueError, match="No reads overlap any transcripts"):
        FM.simplistic_from_counts(np.array([1, 0, 0, 0]), e["hist"])


@pytest.mark.parametrize("m,fallback", [(3000, False), (400, True)])
def test_length_model_from_a_histogram_equals_the_one_from_the_lengths(m, fallback, restated):
    if fallback:
        d = synth_aln.make(60, 400, seed=5)
        e = FR.estimate(d["transcripts"], XB.order_mates(d["fragments"]))
    else:
        e = restated
    lens = e["min_fraglen"][e["min_fraglen"] > 0]
    assert (len(lens) < 1000) == fallback and (lens <= 2000).all()
    a, b = B.fragment_length_model_from_hist(e["hist"]), B.fragment_length_model(lens)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    assert a["fraglen_pmf"].dtype == np.float32 and abs(float(a["fraglen_cdf"][-1]) - 1.0) < 1e-4
    if fallback:
        assert a["fraglen_median"] == 150


def test_subsample_fragments(data):
    T, F = data
    m = F["m"]
    keys = np.stack([np.asarray(F["seq"], np.int64), np.asarray(F["m1_left"], np.int64)], axis=1)
    assert len(np.unique(keys, axis=0)) == 2545
    sub, idx = FM.subsample_fragments(F, 1000, seed=3)
    assert sub["m"] == len(idx) == 1000 and (np.diff(idx) > 0).all()
    assert len(np.unique(keys[idx], axis=0)) == 1000  # chosen keys are distinct
    for i in idx.tolist():  # the lowest index of its key
        assert i == np.flatnonzero((keys == keys[i]).all(axis=1))[0]
    sub2, idx2 = FM.subsample_fragments(F, 1000, seed=3)
    assert (idx == idx2).all() and all(np.array_equal(sub[k], sub2[k]) for k in sub if k != "m")
    assert not np.array_equal(idx, FM.subsample_fragments(F, 1000, seed=4)[1])
    # all keys when there are no more than asked for, whatever the seed
    for N in (2545, 200000):
        _, all_idx = FM.subsample_fragments(F, N, seed=9)
        _, first = np.unique(keys, axis=0, return_index=True)
        assert np.array_equal(all_idx, np.sort(first))
    # fields and CIGAR ranges of the subset read back equal
    for k in ("seq", "strand", "m1_left", "m1_right", "m2_left", "m2_right", "m1_is_flag16"):
        assert np.array_equal(sub[k], np.asarray(F[k])[idx])
    for which in ("cig1_ptr", "cig2_ptr"):
        p, q = np.asarray(F[which]), sub[which]
        assert len(q) == len(idx) + 1
        for r, i in enumerate(idx.tolist()):
            assert np.array_equal(sub["cig_op"][q[r]:q[r + 1]], F["cig_op"][p[i]:p[i + 1]])
            assert np.array_equal(sub["cig_len"][q[r]:q[r + 1]], F["cig_len"][p[i]:p[i + 1]])
    # the subset is a valid input of its own: the restated estimate of it equals the estimate's values at idx
    assert np.array_equal(FR.estimate(T, sub)["min_fraglen"], FR.estimate(T, F)["min_fraglen"][idx])
    assert (FM.subsample_fragments(F, 1, seed=0)[0]["m"], FM.subsample_fragments(F, 0, seed=0)[0]["m"]) == (1, 0)


def test_the_draw_on_hand_rows():
    p = np.array([0.25, 0.75], np.float32) * np.float32(0.5)  # probabilities (0.25, 0.75), exactly
    below, above = np.nextafter(0.25, 0.0), np.nextafter(0.25, 1.0)
    assert FR.draw(p, below) == 0 and FR.draw(p, 0.25) == 1 and FR.draw(p, above) == 1
    # the last entry catches the remainder, even where rounding leaves r above its zj
    assert FR.draw(np.array([0.1, 0.2, 0.3], np.float32), 1.0 - 2.0 ** -53) == 2
    assert FR.draw(np.array([3.0], np.float32), 0.999) == 0
    assert FR.draw(np.zeros(3, np.float32), 0.5) == 2  # (z_sum = 0: every zj is NaN, nothing is taken before the last)
    # as written: the last entry, for any xs and any uniform
    rng = np.random.default_rng(0)
    for _ in range(50):
        k = int(rng.integers(1, 7))
        assert FR.as_written(rng.random(k).astype(np.float32), float(rng.random())) == k - 1
    # 53-bit uniforms: strictly inside (0, 1), exact
    assert FR.u01_53(0, 0) == 2.0 ** -53 and FR.u01_53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
    assert FR.u01_53(1 << 6, 0) == (2.0 ** 26 + 0.5) * 2.0 ** -52


def test_frequency_of_the_first_entry_over_identical_rows():
    N, p0 = 20000, 0.3
    prod = np.array([p0, 1.0 - p0], np.float32)
    us = FR.uniforms(np.arange(N), seed=11)
    assert us.min() > 0.0 and us.max() < 1.0
    z0 = float(prod[0]) / (float(prod[0]) + float(prod[1]))
    first = sum(FR.draw(prod, u) == 0 for u in us)
    assert first == int((us < z0).sum())
    assert abs(first / N - z0) <= 4.0 * math.sqrt(z0 * (1.0 - z0) / N), first / N
    assert not np.array_equal(us, FR.uniforms(np.arange(N), seed=12))
    # fragment ids beyond 32 bits reach the second counter word
    assert FR.uniforms([5], 1)[0] != FR.uniforms([5 + (1 << 32)], 1)[0]


def test_genomic_to_transcriptomic_on_hand_fragments():
    """the interval of the hand-made case's fragments on their transcript (200 bases), overhangs on both ends nudged"""
    T, F = _hand_case()
    I = FR.Inputs(T, F)
    rev = np.zeros(F["m"], np.uint8)
    assert FR.genomic_to_transcriptomic(I, 0, 0, rev, 150) == (11, 170)
    assert FR.genomic_to_transcriptomic(I, 0, 2, rev, 150) == (51, 130)
    assert FR.genomic_to_transcriptomic(I, 0, 5, rev, 150) == (21, 150)   # single-end, forward: from its left end, the fallback length
    assert FR.genomic_to_transcriptomic(I, 0, 5, rev, 190) == (21, 180)   # ... cut at the transcript's end
    rev[5] = 1
    assert FR.genomic_to_transcriptomic(I, 0, 5, rev, 150) == (1, 69)     # reverse: 70 - 150 = -80 -> nudged to 1, 150 - 81 left
    assert FR.genomic_to_transcriptomic(I, 0, 5, rev, 0) == (0, 0)
    assert FR.genomic_to_transcriptomic(I, 0, 6, rev, 150) == (0, 0)      # incompatible
    T["strand"] = np.array([-1], np.int8)
    I = FR.Inputs(T, F)
    assert FR.genomic_to_transcriptomic(I, 0, 0, rev, 150) == (21, 170)   # from its right end, 380 -> 200 - 180 + 1


def test_overhangs_on_both_ends_are_nudged():
    """fragments soft-clipped past an exon's end and single-end reads whose guessed length runs past a transcript end, on both strands"""
    T, F, rev, expected = FR.overhang_case()
    I = FR.Inputs(T, F)
    assert len(expected) == 10
    for (i, j), want in expected.items():
        assert FR.genomic_to_transcriptomic(I, j, i, rev, 150) == want, (i, j)
    assert sum(tpos == 1 for tpos, _ in expected.values()) == 4 and sum(tpos + fl - 1 == 200 for tpos, fl in expected.values()) == 2


def test_command_line_parser_and_model_file(tmp_path, capsys):
    for bad in (["in.npz"], ["in.npz", "-o", "x.npz", "--assign", "nearest"], ["in.npz", "-o", "x.npz", "--mixture", "gibbs"],
                ["in.npz", "-o", "x.npz", "--num-training-reads", "0"], ["in.npz", "-o", "x.npz", "--host"], ["-o", "x.npz"]):
        with pytest.raises(SystemExit) as e:
            FM.main(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    a = FM.parser().parse_args(["in.npz", "-o", "out.npz"])
    assert (a.assign, a.mixture, a.num_training_reads, a.seed, a.device, a.no_bias, a.alt_frag_model) == ("draw", "optimize", 200000, 0, 0, False, False)
    with pytest.raises(ValueError, match="missing t_seq"):
        np.savez(tmp_path / "empty.npz", seq=np.zeros(1, np.int32))
        FM.read_alignments(tmp_path / "empty.npz")
    # alignments.npz round trip
    T, F = _hand_case()
    np.savez(tmp_path / "aln.npz", t_seq=T["seq"], t_strand=T["strand"], tseq_ptr=np.array([0, 200]), tseq=np.zeros(200, np.uint8),
             **{k: T[k] for k in ("exon_ptr", "exon_first", "exon_last")}, **{k: F[k] for k in XB._F_TYPES})
    T2, F2, tp, ts, rev = FM.read_alignments(tmp_path / "aln.npz")
    assert T2["n"] == 1 and F2["m"] == F["m"] and rev is None and all(np.array_equal(F2[k], F[k]) for k in XB._F_TYPES)
    # a model dict round trip, with and without a bias model
    lm = B.fragment_length_model(np.arange(100, 1200))
    fm = dict(fraglen_pmf=lm["fraglen_pmf"], fraglen_cdf=lm["fraglen_cdf"], fraglen_median=lm["fraglen_median"], strand_specificity=0.75,
              alt_frag_model=False)
    bias = dict(lm, orders_left=np.arange(20, dtype=np.int32), gc_bins=np.ones(100, np.float32), accuracy=0.5, tseq_ptr=np.array([0, 7]))
    diag = dict(indices=np.arange(5), counts=dict(compatible_pairs=9, strand_match=3), seconds=dict(estimate=0.25))
    for b in (bias, None):
        FM.save_model(tmp_path / "model.npz", dict(fragmodel=fm, bias=b, diagnostics=diag))
        back = FM.load_model(tmp_path / "model.npz")
        assert (back["bias"] is None) == (b is None)
        for part, want in (("fragmodel", fm), ("bias", b), ("diagnostics", diag)):
            if want is None:
                continue
            assert sorted(back[part]) == sorted(want)
            for k, v in want.items():
                if isinstance(v, dict):
                    assert back[part][k] == v
                else:
                    assert np.array_equal(back[part][k], v), (part, k)


def test_exports_and_symbols():
    import polee_amd as P
    from polee_amd import _lib
    for name in ("train_fragment_model", "estimate_simplistic", "assign_reads", "subsample_fragments"):
        assert getattr(P, name) is getattr(FM, name)
    assert P.fragment_length_model_from_hist is B.fragment_length_model_from_hist
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s

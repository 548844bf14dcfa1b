"""-m gpu: the device path of the splicing features (polee_splice_run, splice_features.hip) against its host twin, array for array, and on
the hand-made loci against the restatement of the reference too (tests/splicing_restatement.py).  Integer work: every comparison is
exact.  The shapes are the smallest at which the kernels take another path: walks of the overlap join on both sides of the
lane / wave threshold and across waves and workgroups, groups that end at a workgroup's edge, genes larger than a wave."""
import json
import os
import sys

import numpy as np
import pytest

import splicing_restatement as R
from conftest import ROOT, random_tree

sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth_annotation  # noqa: E402

pytestmark = pytest.mark.gpu

LOCI = R.hand_made_loci()


def _both(T, gene_of="own"):
    from polee_amd import splicing
    g = T.get("gene_of") if isinstance(gene_of, str) else gene_of
    dev, host = splicing.splicing_features(T, g), splicing.splicing_features(T, g, host=True)
    R.assert_same(dev, host, "device against host")
    for k in ("num_exons", "num_internal_exons", "num_overlapping_pairs"):
        assert dev[k] == host[k], (k, dev[k], host[k])
    return dev


@pytest.fixture(scope="module")
def hand_made():
    T = R.concatenate([LOCI[k] for k in sorted(LOCI)])
    return T, R.splicing_features(T, T["gene_of"])


@pytest.fixture(scope="module")
def generated():
    return synth_annotation.generate(2000, 1)


def test_hand_made_loci(hand_made):
    T, want = hand_made
    R.assert_same(_both(T), want, "device against the restatement")
    R.assert_same(_both(T, None), R.splicing_features(T, None), "without alternative ends")
    for name in ("no_features", "single_exon", "two_exons"):  # (no internal exon, no member row at all)
        R.assert_same(_both(LOCI[name]), R.splicing_features(LOCI[name], LOCI[name]["gene_of"]), name)


def test_generated_annotation_and_two_runs(generated):
    from polee_amd import splicing
    T = generated
    first = _both(T)
    R.assert_same(first, R.splicing_features(T, T["gene_of"]))
    second = splicing.splicing_features(T, T["gene_of"])
    for k in R.ARRAYS:
        assert first[k].tobytes() == second[k].tobytes(), k
    _both(T, None)


def _overlapping_locus(k, seq=0, strand=1, spread=0):
    """k transcripts of three exons whose internal exons all contain [2900, 3000] (spread 0), or of which each overlaps only its next
    few neighbours (spread > 0): boundaries repeat, so alternative sites and retained introns both come out"""
    ts = []
    for i in range(k):
        if spread:
            mid = (10000 + spread * i, 10000 + spread * i + 120 + 7 * (i % 4))
            ts.append((seq, strand, [(100 + (i % 3), 200 + (i % 7)), mid, (mid[1] + 400 + 10 * (i % 5), mid[1] + 900)]))
        else:
            ts.append((seq, strand, [(100, 200 + (i % 7)), (1000 + 3 * i, 3000 + 5 * (i % 11)), (5000 + 10 * (i % 5), 6000)]))
    return ts


def test_one_locus_of_300_mutually_overlapping_exons():
    """every walk but the last 32 is longer than a lane takes alone (the wave's path), the walks cross waves and workgroups, and the
    44 850 pairs give more rows than one thread should carry"""
    ts = _overlapping_locus(300) + _overlapping_locus(40, seq=1, strand=-1)
    T = R.annotation(ts, [1] * len(ts))
    got = _both(T, None)
    assert got["num_overlapping_pairs"] == 300 * 299 // 2 + 40 * 39 // 2
    R.assert_same(got, R.splicing_features(T, None))


@pytest.mark.parametrize("k", [63, 64, 65, 256, 257, 512])
def test_group_sizes_around_the_wave_and_the_workgroup(k):
    """k internal exons in one (sequence, strand) group, chained overlaps (walks of a few exons: the lanes' own path); at 256 and 512 the
    exons, the flanks and the sorted group end exactly where a workgroup does"""
    ts = _overlapping_locus(k, spread=50)
    T = R.annotation(ts, [1] * k)
    assert int(T["exon_ptr"][-1]) == 3 * k
    got = _both(T, None)
    assert got["num_internal_exons"] == k
    R.assert_same(got, R.splicing_features(T, None))
    # the same exons as mutual overlaps: walks of k - 1 down to 0 partners in one group
    T = R.annotation(_overlapping_locus(k), [1] * k)
    R.assert_same(_both(T, None), R.splicing_features(T, None))


@pytest.mark.parametrize("size", [65, 300])
def test_large_genes_for_the_alternative_ends(size):
    """one gene of `size` transcripts (five clusters of starts, two of ends) between two small ones"""
    ts = [(0, 1, [(100, 200), (400, 500)]), (0, 1, [(900, 950), (1400, 1500)])]
    ts += [(1, -1, [(10000 + 1000 * (i % 5) + 3 * (i // 5), 20000), (30000, 31000 + 600 * (i % 2) + (i % 13))]) for i in range(size)]
    ts += [(2, 1, [(100, 200), (400, 500)]), (2, 1, [(120, 200), (400, 900)])]
    genes = [1, 1] + [2] * size + [3, 3]
    order = np.random.default_rng(size).permutation(len(ts))
    T = R.annotation([ts[i] for i in order], [genes[i] for i in order])
    got = _both(T)
    R.assert_same(got, R.splicing_features(T, T["gene_of"]))
    big = got["seq"] == 1
    assert big.sum() == 5 + 1 and (np.diff(got["included_ptr"])[big] + np.diff(got["excluded_ptr"])[big] == size).all()


def test_one_gene_holds_most_transcripts():
    """a gene map gone wrong: 5 000 of 5 004 transcripts in one gene, 40 clusters of starts and two of ends (one thread walks
    that gene and writes its 41 x 5 000 rows)"""
    size = 5000
    ts = [(0, 1, [(100, 200), (400, 500)]), (0, 1, [(900, 950), (1400, 1500)])]
    ts += [(1, 1, [(10000 + 400 * (i % 40) + (i // 40) % 100, 90000), (95000, 96000 + 600 * (i % 2) + (i % 13))]) for i in range(size)]
    ts += [(2, -1, [(100, 200), (400, 500)]), (2, -1, [(120, 200), (400, 900)])]
    genes = [1, 1] + [2] * size + [3, 3]
    order = np.random.default_rng(9).permutation(len(ts))
    T = R.annotation([ts[i] for i in order], [genes[i] for i in order])
    got = _both(T)
    R.assert_same(got, R.splicing_features(T, T["gene_of"]))
    big = got["seq"] == 1
    assert big.sum() == 40 + 1 and (np.diff(got["included_ptr"])[big] + np.diff(got["excluded_ptr"])[big] == size).all()


def test_refusals_name_the_entry():
    from polee_amd import splicing
    from polee_amd._lib import PoleeError
    with pytest.raises(PoleeError, match="polee_splice_run: .*outside"):
        splicing.splicing_features(R.annotation([(0, 1, [(5, 2 ** 31 - 1)])]))
    with pytest.raises(PoleeError, match="polee_splice_run: .*ascend"):
        splicing.splicing_features(R.annotation([(0, 1, [(100, 200), (150, 300)])]))


def test_experiment_path(hand_made, tmp_path):
    """`--experiment`: on synthetic approximations over the hand-made annotation's transcripts the command line's loc / scale equal a
    direct approximate_splicing_likelihood call given the restatement's index pairs and the same seed, and x_init is the log-ratio of
    the summed initial values"""
    from oracle import oracle as O
    from polee_amd import estimate, h5io, splicing
    from polee_amd.core import Context
    T, want = hand_made
    n, S = int(T["n"]), 3
    rng = np.random.default_rng(3)
    tree = random_tree(n, rng)
    to = O.PTT(*tree)
    samples = []
    for i in range(S):
        logx = rng.normal(0, 1.0, size=n)
        x = np.exp(logx - logx.max())
        x /= x.sum()
        yy = np.clip(to.inverse_transform(x.astype(np.float32))[0], 1e-6, 1 - 1e-6)
        fn = str(tmp_path / ("sample%d.h5" % i))
        h5io.write_approximation(fn, 1000000, n, np.full(n, 1000.0, np.float32),
                                 dict(mu=(np.log(yy) - np.log1p(-yy)).astype(np.float32), omega=np.full(n - 1, np.log(0.05), np.float32),
                                      alpha=np.zeros(n - 1, np.float32), node_parent_idxs=tree[0], node_js=tree[1]))
        samples.append({"name": "sample%d" % i, "file": fn, "factors": {"tissue": "ab"[i % 2]}})
    (tmp_path / "experiment.yml").write_text(json.dumps({"samples": samples}))
    ids = ["g%d.t%d" % (g, j) for j, g in enumerate(T["gene_of"])]
    (tmp_path / "ids.txt").write_text("".join(t + "\n" for t in ids))
    np.savez(tmp_path / "transcripts.npz", t_seq=T["seq"], t_strand=T["strand"], exon_ptr=T["exon_ptr"], exon_first=T["exon_first"],
             exon_last=T["exon_last"])
    out, approx = str(tmp_path / "features.npz"), str(tmp_path / "splicing-approx.csv")
    assert splicing.main([str(tmp_path / "transcripts.npz"), "-o", out, "--alt-ends", "--transcript-ids", str(tmp_path / "ids.txt"), "--gene-pattern",
                          r"^(g\d+)\.", "--experiment", str(tmp_path / "experiment.yml"), "--approx-output", approx, "--seed", "7"]) == 0
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    R.assert_same(got, want)
    F = want["num_features"]
    ctx = Context(0)
    ls = estimate.load_samples_from_specification({"samples": samples}, n, ctx=ctx)
    loc, scale = ls.variables["approx"].approximate_splicing_likelihood(
        F, np.stack([want["feature_idxs"] - 1, want["feature_transcript_idxs"] - 1], axis=1),
        np.stack([want["antifeature_idxs"] - 1, want["antifeature_transcript_idxs"] - 1], axis=1), seed=7)
    again = ls.variables["approx"].approximate_splicing_likelihood(
        F, np.stack([want["feature_idxs"] - 1, want["feature_transcript_idxs"] - 1], axis=1),
        np.stack([want["antifeature_idxs"] - 1, want["antifeature_transcript_idxs"] - 1], axis=1), seed=7)
    assert loc.tobytes() == again[0].tobytes() and scale.tobytes() == again[1].tobytes()  # (one seed, two calls: the same bits)
    gl = [ls.variables["approx"].approximate_feature_likelihood(F, want["feature_idxs"], want["feature_transcript_idxs"], 50, 50, seed=7) for _ in range(2)]
    assert gl[0][0].tobytes() == gl[1][0].tobytes() and gl[0][1].tobytes() == gl[1][1].tobytes()
    rows = open(approx).read().splitlines()
    assert rows[0] == "i,j,loc,scale" and len(rows) == S * F + 1
    cells = np.array([[float(v) for v in r.split(",")] for r in rows[1:]])
    assert cells[:, 0].tolist() == np.repeat(np.arange(1, S + 1), F).tolist() and cells[:, 1].tolist() == np.tile(np.arange(1, F + 1), S).tolist()
    assert np.array_equal(cells[:, 2].astype(np.float32).reshape(S, F), loc) and np.array_equal(cells[:, 3].astype(np.float32).reshape(S, F), scale)
    assert np.array_equal(got["qx_feature_loc"], loc) and np.array_equal(got["qx_feature_scale"], scale)
    assert np.isfinite(loc).all() and (scale > 0).all()
    assert np.array_equal(got["x_init"], splicing.feature_initial_values(ls.x0_values, want)) and got["x_init"].shape == (S, F)

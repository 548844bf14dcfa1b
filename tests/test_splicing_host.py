"""The host twin of the splicing features (polee_splice_run_host, `python -m polee_amd.splicing --host`) against the restatement of the
reference (tests/splicing_restatement.py), array for array: integer work, so every comparison is exact.  No GPU is touched."""
import os
import sys

import numpy as np
import pytest

import splicing_restatement as R
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth_annotation  # noqa: E402

SEED = 1  # (chosen on the CPU: the restatement alone meets test_generated_annotation_is_not_degenerate with it)
LOCI = R.hand_made_loci()
# what the restatement must find in each hand-made locus, per strand copy: {type name: count}
EXPECTED = {
    "cassette": {"cassette_exon": 1},
    "mutex_two_unions": {"mutex_exon": 1},
    "mutex_three_unions": {},
    "mutex_merging": {"mutex_exon": 1, "alt": 1},
    "alt_case1_short_first": {"alt": 1},
    "alt_case1_long_first": {"alt": 1},
    "alt_case2_short_first": {"alt": 1},
    "alt_case2_long_first": {"alt": 1},
    "retained_following_and_preceding": {"retained_intron": 1},
    "retained_preceding_only": {"retained_intron": 1},
    "line_780_as_written": {"retained_intron": 1},
    "no_branch": {},
    "single_exon": {"end": 1},
    "two_exons": {},
    "identical_transcripts": {"cassette_exon": 2, "alt": 1},
    "ends_one_cluster": {},
    "ends_two_clusters": {"end": 1},
    "ends_three_clusters": {"end": 6},
    "ends_250_apart": {},
    "ends_251_apart": {"end": 1},
    "ends_min_differs_from_max": {"end": 2},
    "no_features": {},
}


def _host(T, gene_of="own"):
    from polee_amd import splicing
    return splicing.splicing_features(T, T.get("gene_of") if isinstance(gene_of, str) else gene_of, host=True)


def _counts(r):
    c = np.bincount(r["type"], minlength=7)
    out = {"cassette_exon": c[0], "mutex_exon": c[1], "alt": c[2] + c[3], "retained_intron": c[4], "end": c[5] + c[6]}
    return {k: int(v) for k, v in out.items() if v}


@pytest.fixture(scope="module")
def generated():
    T = synth_annotation.generate(2000, SEED)
    return T, R.splicing_features(T, T["gene_of"])


def test_the_entry_points_exist():
    from polee_amd import _lib as L
    for name in ("polee_splice_run", "polee_splice_run_host", "polee_splice_sizes", "polee_splice_get", "polee_splice_destroy"):
        assert hasattr(L.lib(), name), name


@pytest.mark.parametrize("name", sorted(LOCI))
def test_hand_made_locus(name):
    T = LOCI[name]
    want = R.splicing_features(T, T["gene_of"])
    if name in EXPECTED:  # (both strand copies carry the same features)
        assert _counts(want) == {k: 2 * v for k, v in EXPECTED[name].items()}, (name, _counts(want))
    R.assert_same(_host(T), want, name)
    R.assert_same(_host(T, None), R.splicing_features(T, None), name + " without alternative ends")


def test_hand_made_details():
    """what the loci were drawn for, read off the restatement's result"""
    r = R.splicing_features(LOCI["cassette"], None)
    assert r["coords"].tolist() == [[300, 400, 201, 499]] * 2 and r["strand"].tolist() == [1, -1]
    assert r["included_idx"].tolist() == [1, 3] and r["excluded_idx"].tolist() == [2, 4]
    r = R.splicing_features(LOCI["mutex_merging"], None)
    assert r["coords"][r["type"] == 1].tolist() == [[300, 450, 500, 600]] * 2  # (300, 400) and (350, 450) merged
    assert r["stats"]["dropped_mutex_groups"] == 0 and R.splicing_features(LOCI["mutex_three_unions"], None)["stats"]["dropped_mutex_groups"] == 2
    # the two size orders of an alternative site give the same key with the transcripts swapped
    a, b = R.splicing_features(LOCI["alt_case1_short_first"], None), R.splicing_features(LOCI["alt_case1_long_first"], None)
    assert a["coords"].tolist() == b["coords"].tolist() == [[381, 699, 421, 699]] * 2
    assert a["included_idx"].tolist() == [1, 3] and b["included_idx"].tolist() == [2, 4]
    assert a["type"].tolist() == [3, 2]  # (the last exon base moves: a donor site on the plus strand, an acceptor site on the minus strand)
    a = R.splicing_features(LOCI["alt_case2_short_first"], None)
    assert a["coords"].tolist() == [[201, 299, 201, 329]] * 2 and a["type"].tolist() == [2, 3] and a["included_idx"].tolist() == [2, 4]
    r = R.splicing_features(LOCI["line_780_as_written"], None)
    assert r["coords"].tolist() == [[291, 359, -1, -1]] * 2 and r["included_idx"].tolist() == [1, 3]
    r = R.splicing_features(LOCI["identical_transcripts"], None)
    assert r["coords"][1].tolist() == [300, 400, 201, 499]
    assert r["included_idx"][r["included_ptr"][1]:r["included_ptr"][2]].tolist() == [1, 2]  # (two identical transcripts, once each)
    assert r["excluded_idx"][r["excluded_ptr"][1]:r["excluded_ptr"][2]].tolist() == [3, 4]
    T = LOCI["other_seq_or_strand"]
    assert R.splicing_features(T, T["gene_of"])["num_features"] == 0
    T = LOCI["ends_min_differs_from_max"]
    r = R.splicing_features(T, T["gene_of"])
    plus = r["strand"] == 1
    assert r["end_span"][plus].tolist() == [[100, 800]] * 2  # (max_last is the minimum of 800, 1500 and 1600, as upstream computes it)
    assert r["type"][plus].tolist() == [5, 6] and r["type"][~plus].tolist() == [5, 6]
    assert r["coords"][plus].tolist() == [[100, 100, -1, -1], [800, 800, -1, -1]]
    T = LOCI["ends_three_clusters"]
    r = R.splicing_features(T, T["gene_of"])
    plus5 = (r["strand"] == 1) & (r["type"] == 5)
    assert r["coords"][plus5][:, :2].tolist() == [[100, 100], [1000, 1000], [2000, 2100]]


def test_all_hand_made_loci_in_one_annotation():
    T = R.concatenate([LOCI[k] for k in sorted(LOCI)])
    R.assert_same(_host(T), R.splicing_features(T, T["gene_of"]))


def test_generated_annotation_is_not_degenerate(generated):
    T, want = generated
    assert T["n"] == 2000 and set(T["seq"].tolist()) == {0, 1, 2} and set(T["strand"].tolist()) == {-1, 1}
    sizes = np.bincount(T["gene_of"])[1:]
    assert sizes.min() >= 1 and sizes.max() <= 12
    counts = np.bincount(want["type"], minlength=7)
    assert (counts >= 10).all(), counts
    assert want["stats"]["dropped_mutex_groups"] >= 1
    assert want["stats"]["features_with_repeated_members"] >= 1


def test_generated_annotation(generated):
    T, want = generated
    got = _host(T)
    R.assert_same(got, want)
    assert got["num_exons"] == len(T["exon_first"])
    R.assert_same(_host(T, None), R.splicing_features(T, None), "without alternative ends")
    again = _host(T)
    for k in R.ARRAYS:
        assert np.array_equal(got[k], again[k]), k


def test_refusals():
    from polee_amd import splicing
    from polee_amd._lib import PoleeError
    empty = dict(n=0, seq=np.zeros(0, np.int32), strand=np.zeros(0, np.int8), exon_ptr=np.zeros(1, np.int64), exon_first=np.zeros(0, np.int64),
                 exon_last=np.zeros(0, np.int64))
    with pytest.raises(PoleeError, match="no transcripts"):
        splicing.splicing_features(empty, host=True)
    none = dict(empty, n=1, seq=np.zeros(1, np.int32), strand=np.ones(1, np.int8), exon_ptr=np.zeros(2, np.int64))
    with pytest.raises(PoleeError, match="no exons"):
        splicing.splicing_features(none, host=True)
    for exons, word in (([(100, 200), (150, 300)], "ascend"), ([(0, 10)], "outside"), ([(5, 2 ** 31 - 1)], "outside"), ([(2 ** 31 + 5, 2 ** 31 + 9)], "outside")):
        with pytest.raises(PoleeError, match=word):
            splicing.splicing_features(R.annotation([(0, 1, exons)]), host=True)
    top = R.annotation([(0, 1, [(5, 9), (2 ** 31 - 12, 2 ** 31 - 2)])])  # (the largest coordinate there is)
    assert splicing.splicing_features(top, host=True)["num_features"] == 0
    with pytest.raises(PoleeError, match="1-based"):
        splicing.splicing_features(R.annotation([(0, 1, [(5, 9)])]), gene_of=[0], host=True)


def test_command_line(generated, tmp_path):
    from polee_amd import splicing
    T, want = generated
    np.savez(tmp_path / "transcripts.npz", t_seq=T["seq"], t_strand=T["strand"], exon_ptr=T["exon_ptr"], exon_first=T["exon_first"],
             exon_last=T["exon_last"])
    (tmp_path / "ids.txt").write_text("".join(t + "\n" for t in T["transcript_ids"]))
    out, table = str(tmp_path / "features.npz"), str(tmp_path / "features.csv")
    assert splicing.main([str(tmp_path / "transcripts.npz"), "-o", out, "--table", table, "--host", "--alt-ends", "--transcript-ids",
                          str(tmp_path / "ids.txt"), "--gene-pattern", r"^(G\d+)\."]) == 0
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    R.assert_same(got, want)
    assert got["type_names"].tolist() == R.TYPE_NAMES
    rows = open(table).read().splitlines()
    assert rows[0] == "feature_num,type,seqname,strand,included_first,included_last,excluded_first,excluded_last"
    assert len(rows) == want["num_features"] + 1
    for i in (0, len(rows) // 2, len(rows) - 2):
        cells = rows[i + 1].split(",")
        assert cells[0] == str(i + 1) and cells[1] == R.TYPE_NAMES[want["type"][i]] and [int(v) for v in cells[4:]] == want["coords"][i].tolist()
    # without --alt-ends the last two blocks are absent
    assert splicing.main([str(tmp_path / "transcripts.npz"), "-o", out, "--host"]) == 0
    with np.load(out) as z:
        R.assert_same({k: z[k] for k in z.files}, R.splicing_features(T, None))
    with pytest.raises(SystemExit, match="--transcript-ids"):
        splicing.main([str(tmp_path / "transcripts.npz"), "-o", out, "--host", "--alt-ends", "--gene-pattern", "x"])


def test_feature_initial_values_name_the_feature():
    from polee_amd import splicing
    T = LOCI["cassette"]
    r = R.splicing_features(T, None)
    x0 = np.array([[0.1, 0.2, 0.3, 0.4], [0.4, 0.3, 0.2, 0.1]], np.float32)
    x = splicing.feature_initial_values(x0, r)
    assert np.allclose(x, np.log(x0[:, [0, 2]]) - np.log(x0[:, [1, 3]]), rtol=1e-6)
    x0[1, 3] = 0.0
    with pytest.raises(ValueError, match=r"feature 2 \(cassette_exon, sequence 1, 300-400\).*sample 2"):
        splicing.feature_initial_values(x0, r)

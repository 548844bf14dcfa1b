"""`polee fit-tree` without a GPU: the FASTA reader, the restatement against itself (indexed form ==
brute-force definition), the library's host builder (polee_kmer_sketch_host, polee_kmer_tree_host) against the restatement
array for array, the tree file, and the --host command line."""
import gzip
import os
import re

import numpy as np
import pytest

import kmer_tree_restatement as R
from conftest import GOLDEN, ROOT
from polee_amd import _lib as L

FIXTURE = os.path.join(GOLDEN, "transcriptome.fa.gz")
TIE_CASES, tie_case, valid_tree = R.TIE_CASES, R.tie_case, R.valid_tree


@pytest.fixture(scope="module")
def fixture_seqs():
    import polee_amd as P
    return P.read_fasta(FIXTURE)


@pytest.fixture(scope="module")
def fixture_ref(fixture_seqs):
    """the restatement on the fixture, computed once: sketches, tree, statistics"""
    sk = R.sketches(fixture_seqs[1])
    stats = {}
    p, j = R.tree_indexed(sk, stats)
    return dict(sk=sk, parents=p, js=j, stats=stats)


@pytest.fixture(scope="module")
def generated():
    """2 000 generated transcripts (tools/synth_seq.py), short enough to keep the restatement quick"""
    from tools import synth_seq
    return synth_seq.make_transcripts(2000, seed=3, mean_len=400, max_len=3000)


def test_library_and_package_export_the_new_names():
    lib = L.lib()
    for name in ("polee_kmer_sketch", "polee_kmer_sketch_host", "polee_kmer_tree_host", "polee_kmer_tree", "polee_fit_tree",
                 "polee_debug_kmer_edges_count", "polee_debug_kmer_edges_fill"):
        assert hasattr(lib, name), name
    import polee_amd as P
    for name in ("read_fasta", "kmer_sketches", "build_polya_tree_transformation"):
        assert callable(getattr(P, name)), name
    assert callable(P.h5io.write_transformation)
    hdr = open(os.path.join(ROOT, "include", "polee_hip.h")).read()
    from polee_amd import fit_tree
    assert int(re.search(r"#define POLEE_KMER_SKETCH_CHUNK (\d+)", hdr).group(1)) == fit_tree.SKETCH_CHUNK
    assert (int(re.search(r"#define POLEE_KMER_K (\d+)", hdr).group(1)), int(re.search(r"#define POLEE_KMER_H (\d+)", hdr).group(1))) == (R.K, R.H)


def test_read_fasta(tmp_path):
    import polee_amd as P
    text = (">t1 gene=A  some description\nACGTN\nacgt\n\n>t2\n>t3\tx\nGG\nTT\n>t4\nAAAA\n")
    plain = tmp_path / "a.fa"
    plain.write_text(text)
    ids, seqs = P.read_fasta(str(plain))
    assert ids == ["t1", "t2", "t3", "t4"]  # file order; the id stops at the first whitespace
    assert seqs == [b"ACGTNacgt", b"", b"GGTT", b"AAAA"]  # multi-line records joined; lower case and N kept; the empty record kept
    gz = tmp_path / "a.fa.gz"
    with gzip.open(str(gz), "wt") as f:
        f.write(text)
    assert P.read_fasta(str(gz)) == (ids, seqs)
    ids2, seqs2 = P.read_fasta(str(plain), excluded=["t3", "nobody"])
    assert ids2 == ["t1", "t2", "t4"] and seqs2 == [b"ACGTNacgt", b"", b"AAAA"]
    dup = tmp_path / "dup.fa"
    dup.write_text(">a\nAC\n>b\nGG\n>a desc\nTT\n")
    with pytest.raises(ValueError, match="duplicate"):
        P.read_fasta(str(dup))
    # an empty record has an empty sketch and is still a leaf
    sk = P.kmer_sketches(seqs, host=True)
    assert sk.shape == (4, 200) and not sk.any()
    p, j = P.build_polya_tree_transformation(seqs, host=True)
    valid_tree(p, j, 4)


@pytest.mark.parametrize("n", TIE_CASES)
def test_restatement_indexed_tree_is_the_brute_force_tree(n):
    sk = tie_case(n)
    assert sk.shape == (n + 2, 200)
    nz = sk != 0
    assert ((sk - np.uint64(1)) % np.uint64(200) == np.arange(200, dtype=np.uint64)[None, :])[nz].all()  # a value determines its bin
    assert (sk[-2] == sk[0]).all() and not sk[-1].any()  # the duplicated and the all-zero sketch
    pi, ji = R.tree_indexed(sk)
    pb, jb = R.tree_brute(sk)
    np.testing.assert_array_equal(pi, pb)
    np.testing.assert_array_equal(ji, jb)
    valid_tree(pi, ji, n + 2)


def test_restatement_sketch_properties():
    rng = np.random.default_rng(7)
    seq = "".join("ACGT"[i] for i in rng.integers(0, 4, 700))
    seq = seq[:300] + "N" + seq[300:500].lower() + seq[500:]
    s = R.sketch(seq)
    np.testing.assert_array_equal(s, R.sketch(R.revcomp(seq)))  # canonical k-mers: strand does not matter
    nz = s != 0
    assert nz.sum() > 100 and ((s[nz] - np.uint64(1)) % np.uint64(200) == np.flatnonzero(nz).astype(np.uint64)).all()
    assert not R.sketch(seq[:31]).any() and R.sketch(seq[:32]).astype(bool).sum() == 1
    assert R.similarity(s, s) == (int(nz.sum()), int((~nz).sum()))
    np.testing.assert_array_equal(R.union(s, np.zeros(200, np.uint64)), s)


def test_fixture_counts_pin_the_restatement(fixture_seqs, fixture_ref):
    """The figures a scratch prototype of the definition gave on the reference's test transcriptome: a cross-check of the
    restatement itself."""
    ids, seqs = fixture_seqs
    lens = [len(s) for s in seqs]
    assert (len(ids), min(lens), max(lens), sum(lens)) == (313, 58, 8893, 528011)
    filled = (fixture_ref["sk"] != 0).sum(axis=1)
    assert round(filled.mean()) == 188 and filled.min() == 23
    assert fixture_ref["stats"] == dict(initial_pairs=1034, longest_run=15, merges=248, left_for_huffman=65, nodes=625, height=12)


def test_host_sketches_equal_the_restatement(fixture_seqs, fixture_ref, generated):
    import polee_amd as P
    np.testing.assert_array_equal(P.kmer_sketches(fixture_seqs[1], host=True), fixture_ref["sk"])
    np.testing.assert_array_equal(P.kmer_sketches(generated[:300], host=True), R.sketches(generated[:300]))


@pytest.mark.parametrize("n", TIE_CASES)
def test_host_tree_equals_the_restatement_on_tie_heavy_sketches(n):
    import polee_amd as P
    sk = tie_case(n)
    p, j = P.kmer_tree(sk, host=True)
    pr, jr = R.tree_indexed(sk)
    valid_tree(p, j, n + 2)
    np.testing.assert_array_equal(p, pr)
    np.testing.assert_array_equal(j, jr)
    u, v, mat, empt = P.kmer_candidate_edges(sk, host=True)
    assert list(zip(u.tolist(), v.tolist(), mat.tolist(), empt.tolist())) == R.candidate_pairs(sk)


def test_host_tree_equals_the_restatement_on_the_fixture(fixture_ref):
    import polee_amd as P
    p, j = P.kmer_tree(fixture_ref["sk"], host=True)
    valid_tree(p, j, 313)
    np.testing.assert_array_equal(p, fixture_ref["parents"])
    np.testing.assert_array_equal(j, fixture_ref["js"])


def test_host_tree_equals_the_restatement_on_generated_transcripts(generated):
    import polee_amd as P
    sk = P.kmer_sketches(generated, host=True)
    assert (sk.any(axis=1)).sum() > 1900 and (~sk.any(axis=1)).sum() > 5  # short transcripts have empty sketches
    p, j = P.kmer_tree(sk, host=True)
    valid_tree(p, j, 2000)
    pr, jr = R.tree_indexed(sk)
    np.testing.assert_array_equal(p, pr)
    np.testing.assert_array_equal(j, jr)
    p2, j2 = P.build_polya_tree_transformation(generated, host=True)
    np.testing.assert_array_equal(p, p2)
    np.testing.assert_array_equal(j, j2)


def test_malformed_sketches_are_rejected():
    import polee_amd as P
    sk = tie_case(12)
    sk[3, 5] = np.uint64(7 + 1)  # h' = 7 belongs in bin 7, not in bin 5
    with pytest.raises(P.PoleeError, match="outside its bin"):
        P.kmer_tree(sk, host=True)
    with pytest.raises(ValueError):
        P.kmer_tree(np.zeros((0, 200), np.uint64), host=True)


def test_write_transformation_round_trips(tmp_path):
    import polee_amd as P
    from polee_amd import h5io
    sk = tie_case(25)
    p, j = P.kmer_tree(sk, host=True)
    ids = ["ENST%05d.%d" % (i, i % 3) for i in range(26)] + ["txé"]
    fn = str(tmp_path / "tree.h5")
    h5io.write_transformation(fn, p, j, ids, "a.fa -o tree.h5")
    p2, j2 = h5io.read_transformation(fn)
    assert p2.dtype == np.int32 and j2.dtype == np.int32
    np.testing.assert_array_equal(p2, p)
    np.testing.assert_array_equal(j2, j)
    assert h5io.read_transformation_ids(fn) == ids
    with h5io.File(fn) as f:
        assert f.read_attr("metadata", "version") == 1
        assert f.read_attr("metadata", "args") == "a.fa -o tree.h5"
        assert f.read_attr("metadata", "date")[:2] == "20"
    with pytest.raises(ValueError):
        h5io.write_transformation(fn, p, j, ids[:-1])


def test_host_command_on_the_fixture(tmp_path, fixture_seqs, fixture_ref, capsys):
    from polee_amd import fit_tree, h5io
    out = str(tmp_path / "tree.h5")
    assert fit_tree.main([FIXTURE, "-o", out, "--host"]) == 0
    assert "n=313" in capsys.readouterr().out
    p, j = h5io.read_transformation(out)
    np.testing.assert_array_equal(p, fixture_ref["parents"])
    np.testing.assert_array_equal(j, fixture_ref["js"])
    assert h5io.read_transformation_ids(out) == fixture_seqs[0]  # FASTA order
    # --exclude-transcripts: the tree of the remaining ones
    ex = tmp_path / "ex.txt"
    ex.write_text("\n".join(fixture_seqs[0][:13]) + "\n")
    out2 = str(tmp_path / "tree2.h5")
    assert fit_tree.main([FIXTURE, "-o", out2, "--host", "--exclude-transcripts", str(ex)]) == 0
    assert h5io.read_transformation_ids(out2) == fixture_seqs[0][13:]
    p2, j2 = h5io.read_transformation(out2)
    pr, jr = R.tree_indexed(fixture_ref["sk"][13:])
    np.testing.assert_array_equal(p2, pr)
    np.testing.assert_array_equal(j2, jr)
    # upstream's GFF3 + genome form: refused with a message that says why
    capsys.readouterr()
    assert fit_tree.main(["genes.gff3", "genome.fa", "-o", out, "--host"]) != 0
    err = capsys.readouterr().err
    assert "GFF3" in err and "not supported" in err

"""`polee fit-tree --merge rounds` without a GPU ("merge in rounds"): the restatement against itself (edge-list
form == all-pairs definition), the figures a prototype gave, the library's host twin (polee_kmer_tree_rounds_host) against the
restatement array for array, the selection step on crafted keys, the thread count, and the --host command line."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_rounds_cases as K
import kmer_rounds_restatement as Q
import kmer_tree_restatement as R
from conftest import GOLDEN, ROOT
from polee_amd import _lib as L

FIXTURE = os.path.join(GOLDEN, "transcriptome.fa.gz")
STATS = ("rounds", "merges", "left_for_huffman", "reevaluated")


@pytest.fixture(scope="module")
def P():
    import polee_amd
    return polee_amd


@pytest.fixture(scope="module")
def fixture_seqs(P):
    return P.read_fasta(FIXTURE)


@pytest.fixture(scope="module")
def refs(P, fixture_seqs):
    """name -> (sketches, parents, js, stats) of the edge-list restatement, computed once"""
    out = {}
    for name, sk in K.all_cases(P, fixture_seqs).items():
        st = {}
        p, j = Q.rounds_indexed(sk, st)
        out[name] = (sk, p, j, st)
    return out


@pytest.fixture(scope="module")
def generated_sk(P):
    from tools import synth_seq
    return P.kmer_sketches(synth_seq.make_transcripts(2000, seed=3, mean_len=400, max_len=3000), host=True)


def test_hash_and_priority_of_the_restatement():
    with np.errstate(over="ignore"):  # the same arithmetic in uint64 arrays
        lo, hi = np.array([12345], np.uint64), np.array([67890], np.uint64)
        h = lo * np.uint64(0x9E3779B97F4A7C15) ^ (hi * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(0x165667B19E3779F9))
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    assert Q.h32(12345, 67890) == int(h[0]) & 0xFFFFFFFF
    assert 0 <= Q.h32(12345, 67890) < 2**32 and Q.h32(1, 2) != Q.h32(2, 1) and Q.h32(1, 2) != Q.h32(1, 3)
    assert Q.jbits(200, 0) == 0x3F800000 and Q.jbits(1, 0) == int(np.float32(0.005).view(np.uint32))
    # distinct fractions with denominators <= 200 are distinct floats, in the order of the fractions
    fr = sorted({(m * 1.0 / d, Q.jbits(m, 200 - d)) for d in range(1, 201) for m in range(1, d + 1)})
    assert all(a[1] < b[1] for a, b in zip(fr, fr[1:]) if b[0] - a[0] > 1e-12)
    assert Q.priority(3, 9, 10, 0) > Q.priority(1, 2, 9, 0)  # J first
    assert (Q.priority(3, 9, 10, 0) > Q.priority(4, 9, 10, 0)) == (Q.h32(3, 9) > Q.h32(4, 9))  # then the hash


def test_edge_list_form_is_the_definition(refs):
    for name, (sk, p, j, st) in refs.items():
        sb = {}
        pb, jb = Q.rounds_brute(sk, sb)
        np.testing.assert_array_equal(p, pb, err_msg=name)
        np.testing.assert_array_equal(j, jb, err_msg=name)
        assert sb["per_round"] == st["per_round"], name
        R.valid_tree(p, j, len(sk))


def test_figures_pin_the_restatement(refs):
    """what a scratch prototype of the definition gave: a cross-check of the restatement itself"""
    sk, p, j, st = refs["fixture"]
    assert st["per_round"] == [82, 45, 38, 26, 16, 15, 12, 7, 4, 2, 1]
    assert (st["rounds"], st["merges"], st["left_for_huffman"], st["reevaluated"], st["height"]) == (11, 248, 65, 774, 12)
    pg, jg = R.tree_indexed(sk)
    assert not ((p == pg).all() and (j == jg).all())  # not the greedy tree
    assert [refs["ties %d" % n][3]["rounds"] for n in (12, 25, 40, 60)] == [8, 18, 22, 34]
    st = refs["one value shared by 300"][3]
    assert (st["rounds"], st["merges"], st["left_for_huffman"], st["reevaluated"]) == (74, 299, 21, 43211)
    assert refs["all empty"][3]["rounds"] == 0 and refs["n = 1"][3]["left_for_huffman"] == 1
    # the small shapes do what they are there for
    assert refs["four copies of one sketch"][3]["per_round"] == [2, 1] and refs["four copies of one sketch"][3]["reevaluated"] == 1
    assert refs["65 disjoint duplicate pairs"][3]["per_round"] == [65] and refs["65 disjoint duplicate pairs"][3]["left_for_huffman"] == 65
    assert refs["all 200 bins against a single bin"][3]["merges"] == 1 and refs["n = 2, nothing shared"][3]["merges"] == 0
    assert refs["values only in bins 192-199"][3]["merges"] >= 4


def test_host_twin_equals_the_restatement(P, refs):
    for name, (sk, p, j, st) in refs.items():
        got = {}
        ph, jh = P.kmer_tree(sk, host=True, merge="rounds", stats=got)
        R.valid_tree(ph, jh, len(sk))
        np.testing.assert_array_equal(ph, p, err_msg=name)
        np.testing.assert_array_equal(jh, j, err_msg=name)
        assert got == {k: st[k] for k in STATS}, name
    for n in (1, 2):
        sk = R.tie_case(n)[:n]
        ph, jh = P.kmer_tree(sk, host=True, merge="rounds")
        pr, jr = Q.rounds_indexed(sk)
        np.testing.assert_array_equal(ph, pr)
        np.testing.assert_array_equal(jh, jr)


def test_host_twin_on_generated_transcripts(P, generated_sk):
    st, got = {}, {}
    pr, jr = Q.rounds_indexed(generated_sk, st)
    p, j = P.kmer_tree(generated_sk, host=True, merge="rounds", stats=got)
    R.valid_tree(p, j, 2000)
    np.testing.assert_array_equal(p, pr)
    np.testing.assert_array_equal(j, jr)
    assert (st["rounds"], st["merges"], st["left_for_huffman"]) == (18, 1505, 495)
    assert got == {k: st[k] for k in STATS}
    gs = {}
    R.tree_indexed(generated_sk, gs)
    assert (gs["merges"], gs["left_for_huffman"]) == (1506, 494)  # the greedy loop's, for comparison
    # the default did not change, and says so
    pg, jg = P.kmer_tree(generated_sk, host=True)
    pg2, jg2 = P.kmer_tree(generated_sk, host=True, merge="greedy")
    assert pg.tobytes() == pg2.tobytes() and jg.tobytes() == jg2.tobytes() and pg.tobytes() != p.tobytes()
    with pytest.raises(ValueError, match="merge"):
        P.kmer_tree(generated_sk, host=True, merge="round")


def _digest(p, j):
    return hashlib.sha256(np.asarray(p, np.int32).tobytes() + np.asarray(j, np.int32).tobytes()).hexdigest()


def test_tree_does_not_depend_on_the_thread_count(P, refs, generated_sk, tmp_path):
    """the thread count is read once per process, so the one-thread run is a child process.  44 850 edges: several chunks per
    pass on the default count."""
    sk = refs["one value shared by 300"][0]
    np.save(str(tmp_path / "a.npy"), sk)
    np.save(str(tmp_path / "b.npy"), generated_sk)
    code = ("import sys, hashlib, numpy as np; sys.path.insert(0, %r); import polee_amd as P\n"
            "for f in sys.argv[1:]:\n"
            "    p, j = P.kmer_tree(np.load(f), host=True, merge='rounds')\n"
            "    print(hashlib.sha256(p.tobytes() + j.tobytes()).hexdigest())\n" % ROOT)
    env = dict(os.environ, POLEE_HOST_THREADS="1")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path / "a.npy"), str(tmp_path / "b.npy")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    here = [_digest(*P.kmer_tree(s, host=True, merge="rounds")) for s in (sk, generated_sk)]
    assert out.stdout.split() == here
    assert here[0] == _digest(*refs["one value shared by 300"][1:3])


def test_selection_step_on_crafted_keys_host(P):
    for name, (nn, u, v, key, want) in K.crafted_selections().items():
        merged, order = P.kmer_round_select(nn, u, v, key, host=True)
        got = sorted((int(order[e]), (u[e], v[e])) for e in range(len(u)) if merged[e])
        assert [e for _, e in got] == want and [q for q, _ in got] == list(range(len(want))), name
        assert (order[merged == 0] == -1).all(), name
        rm, ro = K.select_reference(np.asarray(u), np.asarray(v), np.asarray(key))
        assert (rm == merged).all() and (ro == order).all(), name
    nn, u, v, key = K.random_selection(np.random.default_rng(9))
    merged, order = P.kmer_round_select(nn, u, v, key, host=True)
    rm, ro = K.select_reference(u, v, key)
    assert merged.sum() > 100 and (rm == merged).all() and (ro == order).all()
    with pytest.raises(P.PoleeError, match="u < v"):
        P.kmer_round_select(4, [2], [2], [5], host=True)


def test_exported_names():
    import re
    lib = L.lib()
    names = ("polee_kmer_tree_rounds_host", "polee_kmer_tree_rounds", "polee_fit_tree_rounds", "polee_debug_kmer_round_select")
    for name in names:
        assert hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "polee_hip.h")).read() + open(os.path.join(ROOT, "include", "polee_hip_debug.h")).read()
    jl = open(os.path.join(ROOT, "julia", "PoleeHIP.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in doc, name
    for name in names[:3]:
        assert (":" + name) in jl, name
    import polee_amd as P
    from polee_amd import fit_tree
    assert callable(P.kmer_round_select) and fit_tree.MERGES == ("greedy", "rounds")


def test_host_command_with_merge_rounds(P, refs, fixture_seqs, tmp_path, capsys):
    from polee_amd import fit_tree, h5io
    out = str(tmp_path / "tree.h5")
    assert fit_tree.main([FIXTURE, "-o", out, "--host", "--merge", "rounds"]) == 0
    line = capsys.readouterr().out
    assert "n=313" in line and "11 rounds" in line
    p, j = h5io.read_transformation(out)
    np.testing.assert_array_equal(p, refs["fixture"][1])
    np.testing.assert_array_equal(j, refs["fixture"][2])
    assert h5io.read_transformation_ids(out) == fixture_seqs[0]
    p2, j2 = P.build_polya_tree_transformation(fixture_seqs[1], host=True, merge="rounds")
    np.testing.assert_array_equal(p, p2)
    np.testing.assert_array_equal(j, j2)
    # the default is the greedy tree, and the line says which method ran
    out2 = str(tmp_path / "tree2.h5")
    assert fit_tree.main([FIXTURE, "-o", out2, "--host"]) == 0
    assert "greedy" in capsys.readouterr().out
    pg, jg = h5io.read_transformation(out2)
    ph, jh = P.kmer_tree(refs["fixture"][0], host=True)
    np.testing.assert_array_equal(pg, ph)
    np.testing.assert_array_equal(jg, jh)

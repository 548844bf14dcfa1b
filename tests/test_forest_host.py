"""Host side of `polee model random-forest` (polee_amd/random_forest.py, csrc/forest_host.cpp): the keyed
bijection, hand cases with known answers, the library's host builder and host votes against the NumPy restatement
(tests/forest_restatement.py) array for array, the command with --host, the kallisto bootstrap path, and the sanitizer driver of the
host builder.  Everything is exact equality.  No GPU."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import forest_restatement as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "polee_amd", "csrc")
NEW_SYMBOLS = ["polee_forest_default_opts", "polee_forest_create", "polee_forest_destroy", "polee_forest_fit_points", "polee_forest_fit",
               "polee_forest_node_count", "polee_forest_get_nodes", "polee_forest_set_nodes", "polee_forest_predict_points",
               "polee_forest_predict", "polee_forest_log_draws", "polee_forest_build_host", "polee_forest_votes_host"]
SHAPES = [(40, 150, 3, 12), (200, 1100, 3, 33), (96, 130, 16, 11)]  # (N, n, k, nsub)


def assert_same_forest(a, b):
    for name, u, v in zip(("tree_off", "feature", "threshold", "left", "right", "label"), a, b):
        assert np.asarray(u).shape == np.asarray(v).shape, name
        np.testing.assert_array_equal(np.asarray(u), np.asarray(v), err_msg=name)  # (thresholds too: bit for bit)


def nsubfeatures_for(n, nsub):
    f = nsub / np.sqrt(n)
    assert R.nsub_of(n, f) == nsub
    return float(f)


def shape_data(shape, seed=0):
    N, n, k, nsub = shape
    x, y = R.planted_data(np.random.default_rng(1000 + N + seed), N, n, k)
    return x, y, nsubfeatures_for(n, nsub)


def depth_of(nodes, t=0):
    off, feature, _, left, right, _ = nodes
    b, depth, level = int(off[t]), 0, [0]
    while True:
        level = [c for i in level if feature[b + i] >= 0 for c in (left[b + i], right[b + i])]
        if not level:
            return depth
        depth += 1


def test_library_and_package_export_the_new_names():
    import polee_amd
    from polee_amd import random_forest as RF
    lib = polee_amd.lib()
    assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert polee_amd.RNASeqRandomForest is RF.RNASeqRandomForest
    for name in ("fit", "fit_sample", "predict", "predict_sample", "nodes", "set_nodes"):
        assert callable(getattr(RF.RNASeqRandomForest, name))
    hdr = open(os.path.join(ROOT, "include", "polee_hip.h")).read()
    assert int(re.search(r"#define POLEE_FOREST_MAX_ROWS (\d+)", hdr).group(1)) == RF.FOREST_MAX_ROWS
    o = RF.forest_opts()
    assert (o.ntrees, o.max_depth, o.min_samples_leaf, o.min_samples_split, o.nsubfeatures, o.partial_sampling) == (200, -1, 1, 2, 10.0, 1.0)
    assert R.nsub_of(200000, 10.0) == 4472 and R.nsub_of(4, 10.0) == 4 and R.nsub_of(1, 10.0) == 1


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 130, 1100])
def test_bijection_hits_every_feature_once(n):
    order = [R.candidate_feature(99, 3, 5, n, pos) for pos in range(n)]
    assert sorted(order) == list(range(n))


def test_bijection_depends_on_node_tree_and_seed():
    a = [R.candidate_feature(99, 3, 5, 130, pos) for pos in range(130)]
    assert a != [R.candidate_feature(99, 3, 6, 130, pos) for pos in range(130)]
    assert a != [R.candidate_feature(99, 4, 5, 130, pos) for pos in range(130)]
    assert a != [R.candidate_feature(98, 3, 5, 130, pos) for pos in range(130)]


def test_bootstrap_is_uniform_enough_and_keeps_duplicates():
    rows = R.bootstrap(5, 2, 40, 40)
    assert rows.min() >= 0 and rows.max() < 40 and len(set(rows.tolist())) < 40
    assert not np.array_equal(rows, R.bootstrap(5, 3, 40, 40))


def _host(x, y, k, seed=1, **kw):
    from polee_amd.random_forest import build_forest_host
    return build_forest_host(x, y, k, seed, **kw)


def _one_tree_on_all_rows(x, y, k, **kw):
    """hand cases must not depend on what the bootstrap drew: find a seed whose tree-0 bootstrap holds every row at least once"""
    N = len(y)
    for seed in range(1, 4000):
        if len(set(R.bootstrap(seed, 0, N, N).tolist())) == N:
            return seed, _host(x, y, k, seed, ntrees=1, **kw), R.build_forest(x, y, k, seed, ntrees=1, **kw)
    raise AssertionError("no seed found")


def test_two_rows_two_classes_split_at_the_midpoint():
    x = np.array([[0.5, 1.0], [0.5, 3.5]], np.float32)
    seed, h, r = _one_tree_on_all_rows(x, [0, 1], 2)
    assert_same_forest(h, r)
    off, feature, thr, left, right, label = h
    assert off.tolist() == [0, 3] and feature.tolist() == [1, -1, -1] and thr[0] == 2.25
    assert left.tolist() == [1, -1, -1] and right.tolist() == [2, -1, -1] and label.tolist() == [0, 0, 1]


def test_a_duplicated_column_goes_to_the_smaller_position():
    rng = np.random.default_rng(3)
    col = rng.normal(size=6).astype(np.float32)
    x = np.stack([col, col], axis=1)
    y = (col > np.median(col)).astype(np.int32)
    seed, h, r = _one_tree_on_all_rows(x, y, 2, max_depth=1)
    assert_same_forest(h, r)
    assert h[1][0] == R.candidate_feature(seed, 0, 0, 2, 0)


def test_no_boundary_between_equal_values():
    rng = np.random.default_rng(4)
    x = np.round(rng.normal(size=(30, 3)), 1).astype(np.float32)  # equal values carry different labels
    y = rng.integers(0, 2, 30).astype(np.int32)
    h, r = _host(x, y, 2, 6, ntrees=1), R.build_forest(x, y, 2, 6, ntrees=1)  # (whatever the bootstrap drew)
    assert_same_forest(h, r)
    off, feature, thr, left, right, label = h
    values =[set(x[:, j].astype(np.float64).tolist()) for j in range(3)]
    internal = feature >= 0
    assert internal.any()
    assert all(t not in values[f] for f, t in zip(feature[internal], thr[internal]))
    # leaves may stay impure: rows that agree in every feature cannot be told apart
    assert R.votes(h, x, 2).sum() == 30


def test_constant_candidates_leave_an_impure_leaf_with_the_smallest_class():
    x = np.full((4, 3), 0.25, np.float32)
    seed, h, r = _one_tree_on_all_rows(x, [2, 1, 1, 2], 3)
    assert_same_forest(h, r)
    assert h[0].tolist() == [0, 1] and h[1].tolist() == [-1] and h[5].tolist() == [1]  # tie of classes 1 and 2


def test_max_depth_and_min_samples_leaf():
    x, y, f = shape_data(SHAPES[0])
    for depth in (0, 1):
        h = _host(x, y, 3, 5, ntrees=3, nsubfeatures=f, max_depth=depth)
        assert_same_forest(h, R.build_forest(x, y, 3, 5, ntrees=3, nsubfeatures=f, max_depth=depth))
        assert all(depth_of(h, t) == depth for t in range(3)) and len(h[1]) == 3 * (1 if depth == 0 else 3)
    h = _host(x, y, 3, 5, ntrees=2, nsubfeatures=f, min_samples_leaf=3)
    assert_same_forest(h, R.build_forest(x, y, 3, 5, ntrees=2, nsubfeatures=f, min_samples_leaf=3))
    # every leaf of a tree holds at least three bootstrap rows
    for t in range(2):
        rows = R.bootstrap(5, t, 40, 40)
        reached = np.zeros(int(h[0][t + 1] - h[0][t]), np.int64)
        one = tuple(a[h[0][t]:h[0][t + 1]] for a in h[1:])
        for r_ in rows:
            i = 0
            while one[0][i] >= 0:
                i = one[2][i] if float(x[r_, one[0][i]]) < one[1][i] else one[3][i]
            reached[i] += 1
        assert (reached[one[0] < 0] >= 3).all()


@pytest.mark.parametrize("partial_sampling", [1.0, 0.7])
@pytest.mark.parametrize("ntrees", [1, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_builder_equals_the_restatement(shape, ntrees, partial_sampling):
    N, n, k, nsub = shape
    x, y, f = shape_data(shape)
    h = _host(x, y, k, 11, ntrees=ntrees, nsubfeatures=f, partial_sampling=partial_sampling)
    r = R.build_forest(x, y, k, 11, ntrees=ntrees, nsubfeatures=f, partial_sampling=partial_sampling)
    assert_same_forest(h, r)
    assert len(h[1]) >= 3 * ntrees and depth_of(h) >= 2


@pytest.mark.parametrize("shape", SHAPES)
def test_host_votes_equal_the_restatement(shape):
    from polee_amd.random_forest import forest_votes_host
    N, n, k, nsub = shape
    x, y, f = shape_data(shape)
    h = _host(x, y, k, 11, ntrees=7, nsubfeatures=f)
    xt, yt = R.planted_data(np.random.default_rng(77), 23, n, k)
    internal = np.flatnonzero(h[1] >= 0)
    # a test row whose value equals a threshold exactly, where a threshold is a float: it goes right
    i = next((i for i in internal if np.float32(h[2][i]) == h[2][i]), None)
    if i is not None:
        xt[0, h[1][i]] = np.float32(h[2][i])
    xt[1] = x[0]  # ... and a training row
    v = forest_votes_host(h, xt, k)
    np.testing.assert_array_equal(v, R.votes(h, xt, k))
    assert (v.sum(axis=1) == 7).all()


def test_host_builder_refuses_bad_input():
    from polee_amd import NonFiniteError, PoleeError
    x, y, f = shape_data(SHAPES[0])
    bad = x.copy()
    bad[3, 4] = -np.inf
    with pytest.raises(NonFiniteError):
        _host(bad, y, 3)
    with pytest.raises(PoleeError):
        _host(x, np.where(y == 0, 3, y), 3)
    with pytest.raises(PoleeError) as ei:
        _host(np.zeros((8193, 1), np.float32), np.zeros(8193, np.int32), 2, ntrees=1)
    assert ei.value.status == 5
    with pytest.raises(PoleeError):
        _host(x, y, 17)


# ---- the command
def _write_experiment(tmp_path, name, x_tpm, classes, ids):
    samples = []
    for i, (row, c) in enumerate(zip(x_tpm, classes)):
        fn = tmp_path / ("%s%d.csv" % (name, i))
        fn.write_text("transcript_id,tpm\n" + "".join("%s,%r\n" % (t, float(v)) for t, v in zip(ids, row)))
        samples.append({"name": "%s%d" % (name, i), "point-estimates": {"est": str(fn)}, "factors": {"tissue": "c%d" % c}})
    yml = tmp_path / (name + ".yml")
    yml.write_text(json.dumps({"samples": samples}))
    return str(yml)


def test_host_command_on_point_estimates(tmp_path):
    from polee_amd import classify, random_forest
    N, n, k = 60, 40, 3
    # (data seed picked so that the restatement reaches 0.9 on the held-out rows: 60 training rows of closed compositions are few)
    lx, y = R.planted_data(np.random.default_rng(34), N + 60, n, k, constant=2)
    tpm = np.exp(lx.astype(np.float64))
    tpm = tpm / tpm.sum(axis=1, keepdims=True) * 1e6
    y[:k] = np.arange(k)  # (every class is in the training set)
    ids = ["t%d" % j for j in range(n)]
    (tmp_path / "ids.txt").write_text("\n".join(ids) + "\n")
    train = _write_experiment(tmp_path, "train", tpm[:N], y[:N], ids)
    test = _write_experiment(tmp_path, "test", tpm[N:], y[N:], ids)
    out_p, out_t = str(tmp_path / "yp.csv"), str(tmp_path / "yt.csv")
    seed = 12345
    assert random_forest.main([train, test, "tissue", "--host", "--point-estimates", "est", "--transcript-ids", str(tmp_path / "ids.txt"),
                               "--ntrees", "50", "--seed", str(seed), "--output-predictions", out_p, "--output-truth", out_t]) == 0
    # the restatement on the rows the command read
    fn = lambda name, cnt: [str(tmp_path / ("%s%d.csv" % (name, i))) for i in range(cnt)]
    x_train = classify.log_point_estimates(classify.load_point_estimates(fn("train", N), ids))
    x_test = classify.log_point_estimates(classify.load_point_estimates(fn("test", 60), ids))
    nodes = R.build_forest(x_train, y[:N], k, seed + 1, ntrees=50)
    probs = R.votes(nodes, x_test, k) / 50.0
    assert (probs.argmax(axis=1) == y[N:]).mean() >= 0.9  # (the definition learns; nothing more is claimed)
    ref_p, ref_t = str(tmp_path / "rp.csv"), str(tmp_path / "rt.csv")
    onehot = np.eye(k, dtype=np.float32)[y[N:]]
    classify.write_classification_probs(["c0", "c1", "c2"], ref_p, ref_t, probs, onehot)
    assert open(out_p).read() == open(ref_p).read() and open(out_t).read() == open(ref_t).read()


@pytest.mark.parametrize("extra,needle", [
    (["--genes"], "--genes is not built"),
    (["--kallisto", "--kallisto-bootstrap"], "Only one of '--kallisto' and '--kallisto-bootstrap'"),
    (["--kallisto", "--point-estimates", "k"], "not compatible"),
    (["--kallisto-bootstrap", "--point-estimates", "k"], "not compatible"),
    (["--pseudocount", "1"], "--pseudocount argument only valid with"),
    (["--point-estimates", "k"], "needs --transcript-ids"),
    (["--host"], "--host takes a point mode"),
])
def test_command_argument_errors(extra, needle):
    from polee_amd import random_forest
    with pytest.raises(SystemExit) as ei:  # (before the experiment files are opened: they do not exist)
        random_forest.main(["train.yml", "test.yml", "tissue"] + extra)
    assert needle in str(ei.value.code)


def test_command_defaults():
    from polee_amd import random_forest
    a = random_forest.parser().parse_args(["train.yml", "test.yml", "tissue"])
    assert (a.ntrees, a.nsubfeatures, a.partial_sampling, a.training_samples, a.testing_samples, a.seed) == (200, 10.0, 1.0, 20, 20, 12345)
    assert (a.output_predictions, a.output_truth, a.max_depth, a.min_samples_leaf, a.host, a.device) == ("y-predicted.csv", "y-true.csv",
                                                                                                    -1, 1, False, 0)


def test_kallisto_bootstrap_path(tmp_path):
    """generated kallisto files with unequal bootstrap counts through the command, against the same arithmetic in NumPy"""
    from polee_amd import classify, h5io, random_forest
    rng = np.random.default_rng(8)
    n, k = 30, 2
    eff = rng.uniform(100, 300, n)
    specs = {}
    truth = {}
    for name, S in (("train", 8), ("test", 5)):
        samples = []
        for s in range(S):
            c = s % k
            fn = str(tmp_path / ("%s%d.h5" % (name, s)))
            counts = [rng.gamma(2.0, 50.0, n) * np.where(np.arange(n) // 3 == c, 6.0, 1.0) for _ in range(2 + (s * 7) % 4)]
            with h5io.File(fn, "w") as f:
                f.create_group("aux")
                f.create_group("bootstrap")
                f.write("aux/eff_lengths", eff)
                f.write("est_counts", counts[0])
                for i, b in enumerate(counts):
                    f.write("bootstrap/bs%d" % i, b)
            truth[fn] = counts
            samples.append({"name": "%s%d" % (name, s), "kallisto": fn, "factors": {"tissue": "c%d" % c}})
        specs[name] = samples
        (tmp_path / (name + ".yml")).write_text(json.dumps({"samples": samples}))
    out_p, out_t = str(tmp_path / "yp.csv"), str(tmp_path / "yt.csv")
    assert random_forest.main([str(tmp_path / "train.yml"), str(tmp_path / "test.yml"), "tissue", "--host", "--kallisto-bootstrap",
                               "--pseudocount", "1", "--ntrees", "9", "--seed", "4", "--output-predictions", out_p,
                               "--output-truth", out_t]) == 0
    logp = lambda b: classify.counts_to_feature_log_props(np.asarray(b, np.float32), eff, 1.0)[0]
    boots = {name: [np.stack([logp(b) for b in truth[s["kallisto"]]]) for s in specs[name]] for name in specs}
    assert len({b.shape[0] for b in boots["test"]}) > 1  # unequal counts
    x = np.concatenate(boots["train"])
    y = np.concatenate([np.full(b.shape[0], s % k) for s, b in enumerate(boots["train"])])
    nodes = R.build_forest(x, y, k, 5, ntrees=9)
    passes = max(b.shape[0] for b in boots["test"])
    acc = np.zeros((5, k))
    for i in range(passes):
        acc += R.votes(nodes, np.stack([b[i % b.shape[0]] for b in boots["test"]]), k) / 9.0
    ref_p, ref_t = str(tmp_path / "rp.csv"), str(tmp_path / "rt.csv")
    classify.write_classification_probs(["c0", "c1"], ref_p, ref_t, acc / passes, np.eye(k, dtype=np.float32)[np.arange(5) % k])
    assert open(out_p).read() == open(ref_p).read() and open(out_t).read() == open(ref_t).read()


def test_host_builder_clean_under_sanitizer():
    """tests/san/forest_main.cpp: a stand-alone driver, built host-only with address,undefined and run on the CPU"""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    subprocess.check_call(["make", "-s", "-C", CSRC, "_obj/san_address_undefined/forest_check", "SAN=address,undefined"],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", POLEE_HOST_THREADS="4")
    r = subprocess.run([os.path.join(CSRC, "_obj", "san_address_undefined", "forest_check")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ok" in r.stdout

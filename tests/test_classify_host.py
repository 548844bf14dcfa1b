"""Host side of `polee model classify` (polee_amd/classify.py; models/classify.jl, models/polee_classify.py): classes, writers, the
point-estimate readers, the command line, and the restatement the GPU tests compare against (its analytic gradients against central
differences of its own loss).  No GPU."""
import json

import numpy as np
import pytest

NEW_SYMBOLS = ["polee_classify_default_opts", "polee_classify_create", "polee_classify_destroy", "polee_classify_set_opts",
               "polee_classify_get_params", "polee_classify_set_params", "polee_classify_reset", "polee_classify_init_bias",
               "polee_classify_init_bias_points", "polee_classify_eval", "polee_classify_eval_points", "polee_classify_fit",
               "polee_classify_fit_points", "polee_classify_predict", "polee_classify_predict_points"]


def test_the_library_exports_the_symbols_and_the_package_the_class():
    import polee_amd
    from polee_amd.classify import RNASeqLogisticRegression, build_factor_matrix
    lib = polee_amd.lib()
    assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert polee_amd.RNASeqLogisticRegression is RNASeqLogisticRegression
    assert polee_amd.build_factor_matrix is build_factor_matrix
    for name in ("fit_sample", "fit", "predict_sample", "predict", "eval_sample", "eval", "loss_and_gradients", "get_params",
                 "set_params"):
        assert callable(getattr(RNASeqLogisticRegression, name))
    import inspect  # (the reference's keywords keep the handle's options unless the caller passes a value)
    assert inspect.signature(RNASeqLogisticRegression.fit_sample).parameters["samples_per_iter"].default is None
    assert inspect.signature(RNASeqLogisticRegression.fit).parameters["loss_scale"].default is None


def test_default_options_are_the_references():
    import ctypes as C
    import polee_amd
    from polee_amd.classify import ClassifyOpts
    o = ClassifyOpts()
    f = polee_amd.lib().polee_classify_default_opts
    f.restype = None
    f(C.byref(o))
    assert o.draws_per_step == 5
    got = np.array([o.learning_rate, o.l1_penalty, o.loss_scale, o.beta1, o.beta2, o.epsilon], np.float32)
    np.testing.assert_array_equal(got, np.array([1e-4, 1e-3, 1.0, 0.9, 0.999, 1e-7], np.float32))


def test_restatement_gradients_match_central_differences():
    """tests/classify_restatement.py in float64 at S = 4, n = 30, k = 3, D = 2, loss_scale 0.7; every entry of w is away from 0, where
    |w| has no derivative."""
    import classify_restatement as T
    rng = np.random.default_rng(71)
    S, n, k, D, l1, ls = 4, 30, 3, 2, 1e-3, 0.7
    lx = rng.normal(-np.log(n), 1.5, size=(D, S, n))
    w = rng.normal(0, 0.1, size=(n, k))
    w[np.abs(w) < 1e-2] = 0.05
    xb = lx[0].mean(axis=0) + rng.normal(0, 0.3, size=n)
    zb = rng.normal(0, 0.5, size=k)
    labels = np.eye(k)[rng.integers(0, k, size=S)]
    loss, g_w, g_xb, g_zb = T.loss_and_gradients(w, xb, zb, lx, labels, l1, ls)
    assert loss == T.loss(w, xb, zb, lx, labels, l1, ls)
    h = 1e-5
    for name, p, g in (("w", w, g_w), ("x_bias", xb, g_xb), ("z_bias", zb, g_zb)):
        scale = np.abs(g).max()
        for idx in np.ndindex(*p.shape):
            keep = p[idx]
            p[idx] = keep + h
            up = T.loss(w, xb, zb, lx, labels, l1, ls)
            p[idx] = keep - h
            dn = T.loss(w, xb, zb, lx, labels, l1, ls)
            p[idx] = keep
            fd = (up - dn) / (2 * h)
            assert abs(g[idx] - fd) <= 1e-5 * abs(fd) + 1e-5 * scale, (name, idx, g[idx], fd)


def test_restatement_adam_and_predict():
    import classify_restatement as T
    p, m, v = T.adam_step(np.array([1.0, -2.0]), np.array([0.5, -4.0]), 0.0, 0.0, 1, 1e-2)
    # (the first step moves every entry by lr, whatever the size of its gradient -- up to eps / sqrt(v) = 1e-7 / 0.0158 of lr)
    np.testing.assert_allclose(p, [1.0 - 1e-2, -2.0 + 1e-2], rtol=0, atol=1e-7)
    np.testing.assert_allclose(m, [0.05, -0.4])
    np.testing.assert_allclose(v, [0.00025, 0.016])
    pr = T.predict(np.zeros((5, 3)), np.zeros(5), np.zeros(3), np.ones((2, 4, 5)))
    np.testing.assert_allclose(pr, np.full((4, 3), 1 / 3))


def test_build_factor_matrix_sorted_classes_reuse_and_unseen_option():
    from polee_amd.classify import build_factor_matrix, factor_names_of
    train = [{"tissue": "liver"}, {"tissue": "brain"}, {"tissue": "liver", "sex": "f"}, {"tissue": "heart"}]
    F, idx = build_factor_matrix(4, train, "tissue")
    assert idx == {"brain": 0, "heart": 1, "liver": 2} and factor_names_of(idx) == ["brain", "heart", "liver"]
    assert F.dtype == np.float32
    np.testing.assert_array_equal(F, [[0, 0, 1], [1, 0, 0], [0, 0, 1], [0, 1, 0]])
    test = [{"tissue": "heart"}, {"tissue": "kidney"}, {}]
    Ft, idx2 = build_factor_matrix(3, test, "tissue", idx)
    assert idx2 is idx
    np.testing.assert_array_equal(Ft, [[0, 1, 0], [0, 0, 0], [0, 0, 0]])  # (unseen option, missing factor: all-zero rows)
    Fm, idxm = build_factor_matrix(2, [{"a": "x"}, {}], "a")  # (string(missing) is an option of its own in the training set)
    assert idxm == {"missing": 0, "x": 1}
    np.testing.assert_array_equal(Fm, [[0, 1], [1, 0]])
    with pytest.raises(ValueError):
        build_factor_matrix(3, train, "tissue")


def test_writers_byte_for_byte(tmp_path):
    from polee_amd import classify
    yp = np.array([[0.75, 0.25], [1e-5, 0.99999]], np.float32)
    yt = np.array([[1, 0], [0, 0]], np.float32)
    classify.write_classification_probs(["brain", "liver"], str(tmp_path / "p.csv"), str(tmp_path / "t.csv"), yp, yt)
    assert (tmp_path / "p.csv").read_bytes() == b"brain,liver\n0.75,0.25\n1.0e-5,0.99999\n"
    assert (tmp_path / "t.csv").read_bytes() == b"brain,liver\n1.0,0.0\n0.0,0.0\n"
    classify.write_w(str(tmp_path / "w.csv"), np.array([[0.5, -1.25], [0.0, 3e-7], [2.0, 0.1]], np.float32))
    assert (tmp_path / "w.csv").read_bytes() == b"0.5\t-1.25\n0.0\t3.0e-7\n2.0\t0.1\n"
    with pytest.raises(ValueError):
        classify.write_classification_probs(["a"], str(tmp_path / "x.csv"), str(tmp_path / "y.csv"), yp, yt)


def test_point_estimate_csv_reader_and_pseudocount(tmp_path):
    from polee_amd import classify
    (tmp_path / "a.csv").write_text("transcript_id,tpm\nt2,250000.0\nunknown,5.0\nt1,750000.0\n")
    (tmp_path / "b.csv").write_text("transcript_id,tpm\nt3,1000000\n")
    x0 = classify.load_point_estimates([str(tmp_path / "a.csv"), str(tmp_path / "b.csv")], ["t1", "t2", "t3"])
    assert x0.dtype == np.float32
    np.testing.assert_array_equal(x0, np.array([[0.75, 0.25, 0.0], [0.0, 0.0, 1.0]], np.float32))
    lx = classify.log_point_estimates(x0)
    assert np.isneginf(lx[0, 2]) and lx[1, 2] == 0.0  # (log 0, as the reference takes it)
    lp = classify.log_point_estimates(x0, 1.0)
    assert np.isfinite(lp).all()
    # (Float32 throughout, as the reference: the sum is rounded to 6e-8 relative before the log)
    np.testing.assert_allclose(np.exp(lp.astype(np.float64)), np.array([[0.75, 0.25, 0.0], [0.0, 0.0, 1.0]]) + 1e-6, rtol=3e-7)
    (tmp_path / "bad.csv").write_text("id,tpm\nt1,1\n")
    with pytest.raises(ValueError):
        classify.load_point_estimates([str(tmp_path / "bad.csv")], ["t1"])


def test_kallisto_reader_round_trip(tmp_path):
    """a file written by polee_amd.sample.write_kallisto read back through read_kallisto_estimates (models/kallisto.jl:2-26)"""
    from polee_amd import classify
    from polee_amd.sample import write_kallisto
    est = np.array([10.0, 0.0, 30.0, 60.0])
    eff = np.array([100.0, 200.0, 300.0, 150.0])
    fn = str(tmp_path / "k.h5")
    write_kallisto(fn, [np.zeros((1, 4))], est, eff, ["a", "b", "c", "d"], [1, 2, 3, 4])
    lx = classify.read_kallisto_estimates([fn, fn], pseudocount=2.0)
    assert lx.shape == (2, 4) and lx.dtype == np.float32
    t = est / eff
    np.testing.assert_allclose(lx[0], np.log(t / t.sum() + 2e-6), rtol=1e-6)
    np.testing.assert_array_equal(lx[0], lx[1])
    assert np.isneginf(classify.read_kallisto_estimates([fn])[0, 1])


def test_cli_defaults_and_options():
    from polee_amd import classify
    a = classify.parser().parse_args(["train.yml", "test.yml", "tissue"])
    assert (a.training_experiment, a.testing_experiment, a.factor) == ("train.yml", "test.yml", "tissue")
    assert (a.output_predictions, a.output_truth, a.output_w) == ("y-predicted.csv", "y-true.csv", "w.csv")
    assert (a.num_steps, a.testing_samples, a.draws_per_step, a.learning_rate, a.device) == (5000, 100, 5, 1e-4, 0)
    assert (a.point_estimates, a.kallisto, a.pseudocount, a.transcript_ids, a.feature) == (None, False, None, None, "transcript")
    a = classify.parser().parse_args(["a", "b", "f", "--point-estimates", "salmon", "--pseudocount", "0.5", "--num-steps", "7",
                                      "--testing-samples", "3", "--draws-per-step", "2", "--learning-rate", "0.01", "--seed", "9",
                                      "--device", "1", "--transcript-ids", "ids.txt", "--output-w", "ww.csv"])
    assert (a.point_estimates, a.pseudocount, a.num_steps, a.testing_samples, a.draws_per_step, a.learning_rate, a.seed, a.device,
            a.transcript_ids, a.output_w) == ("salmon", 0.5, 7, 3, 2, 0.01, 9, 1, "ids.txt", "ww.csv")
    with pytest.raises(SystemExit):
        classify.parser().parse_args(["train.yml", "test.yml"])


@pytest.mark.parametrize("extra,needle", [
    (["--kallisto-bootstrap"], "--kallisto-bootstrap is not built"),
    (["--feature", "gene"], "--feature gene is not built"),
    (["--feature", "splicing"], "--feature splicing is not built"),
    (["--pseudocount", "1"], "--pseudocount argument only valid with"),
    (["--kallisto", "--kallisto-bootstrap"], "Only one of '--kallisto' and '--kallisto-bootstrap'"),
    (["--kallisto", "--point-estimates", "k"], "not compatible"),
    (["--point-estimates", "k"], "needs --transcript-ids"),
])
def test_cli_refuses_what_is_not_built(extra, needle):
    from polee_amd import classify
    with pytest.raises(SystemExit) as ei:  # (before the experiment files are opened: they do not exist)
        classify.main(["train.yml", "test.yml", "tissue"] + extra)
    assert needle in str(ei.value.code)


def test_experiment_files_are_read_as_pca_reads_them(tmp_path):
    from polee_amd import classify, estimate, pca
    spec = {"samples": [{"name": "a", "file": "a.h5", "factors": {"tissue": "liver"}}, {"name": "b", "factors": {"tissue": 1}}]}
    f = tmp_path / "e.yml"
    f.write_text(json.dumps(spec))
    _, names, factors = estimate.read_specification(pca.read_experiment(str(f)))
    F, idx = classify.build_factor_matrix(2, factors, "tissue")
    assert names == ["a", "b"] and idx == {"1": 0, "liver": 1}
    np.testing.assert_array_equal(F, [[0, 1], [1, 0]])

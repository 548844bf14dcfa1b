"""Host side of `polee model tsne` (polee_amd/tsne.py; models/tsne.jl, models/polee_tsne.py): the exports, the command line, the
writer, the seed rules, find_sigmas, and the restatement the GPU tests compare against (its analytic gradient against central
differences of its own loss).  No GPU."""
import numpy as np
import pytest

NEW_SYMBOLS = ["polee_tsne_default_opts", "polee_tsne_create", "polee_tsne_destroy", "polee_tsne_get_params", "polee_tsne_set_params",
               "polee_tsne_reset", "polee_tsne_set_sigmas", "polee_tsne_distances", "polee_tsne_distances_points", "polee_tsne_eval",
               "polee_tsne_eval_points", "polee_tsne_fit", "polee_tsne_fit_points", "polee_tsne_embed", "polee_tsne_embed_points"]


def test_the_library_exports_the_symbols_and_the_package_the_class():
    import polee_amd
    from polee_amd.tsne import RNASeqTSNE, estimate_tsne
    lib = polee_amd.lib()
    assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert polee_amd.RNASeqTSNE is RNASeqTSNE and polee_amd.estimate_tsne is estimate_tsne
    for name in ("distances", "find_sigmas", "set_sigmas", "loss_and_gradient", "fit", "embed", "get_params", "set_params"):
        assert callable(getattr(RNASeqTSNE, name))


def test_default_options_are_the_references():
    import ctypes as C
    import polee_amd
    from polee_amd.tsne import TSNEOpts
    o = TSNEOpts()
    f = polee_amd.lib().polee_tsne_default_opts
    f.restype = None
    f(C.byref(o))
    assert (o.num_components, o.use_vlr) == (2, 1)
    got = np.array([o.alpha, o.eps, o.learning_rate, o.beta1, o.beta2, o.epsilon], np.float32)
    np.testing.assert_array_equal(got, np.array([1.0, 1e-6, 1e-6, 0.99, 0.999, 1e-8], np.float32))


def test_cli_defaults_and_options():
    from polee_amd import tsne
    a = tsne.parser().parse_args(["experiment.yml"])
    assert (a.experiment, a.feature, a.num_components, a.posterior_mean, a.output_z, a.max_num_samples, a.batch_size) == \
        ("experiment.yml", "transcript", 2, False, "tsne-z.csv", None, 100)
    assert (a.num_steps, a.perplexity, a.learning_rate, a.l2, a.device, a.transcript_ids) == (500, 50.0, 1e-6, False, 0, None)
    a = tsne.parser().parse_args(["e.yml", "--num-components", "3", "--posterior-mean", "--output-z", "z.csv", "--max-num-samples", "9",
                                  "--batch-size", "7", "--num-steps", "11", "--perplexity", "4", "--learning-rate", "1e-3", "--l2",
                                  "--seed", "5", "--device", "1", "--transcript-ids", "ids.txt"])
    assert (a.num_components, a.posterior_mean, a.output_z, a.max_num_samples, a.batch_size, a.num_steps, a.perplexity, a.learning_rate,
            a.l2, a.seed, a.device, a.transcript_ids) == (3, True, "z.csv", 9, 7, 11, 4.0, 1e-3, True, 5, 1, "ids.txt")
    with pytest.raises(SystemExit):
        tsne.parser().parse_args([])


@pytest.mark.parametrize("feature,needle", [("gene", "gene feature is not yet implemented."),
                                            ("splicing", "splicing feature is not yet implemented."),
                                            ("exon", "exon is not a supported feature.")])
def test_cli_refuses_the_features_the_reference_refuses(feature, needle):
    from polee_amd import tsne
    with pytest.raises(SystemExit) as ei:  # (before the experiment file is opened: it does not exist)
        tsne.main(["experiment.yml", "--feature", feature])
    assert str(ei.value.code) == needle


def test_the_csv_is_byte_for_byte_the_writers(tmp_path):
    from polee_amd.pca import write_pca_z
    z = np.array([[0.5, -1.25], [3e-7, 2.0], [123456.0, 1e7]], np.float32)
    write_pca_z(str(tmp_path / "tsne-z.csv"), ["a", "b", "c"], z)
    assert (tmp_path / "tsne-z.csv").read_bytes() == b"sample,component1,component2\na,0.5,-1.25\nb,3.0e-7,2.0\nc,123456.0,1.0e7\n"


def _problem(rng, S, n, C):
    """a shared profile, two groups of samples and per-sample noise of graded size, so that the pairwise distances differ by an
    order of magnitude"""
    group = (np.arange(S) % 2)[:, None] * rng.normal(0, 0.7, size=(1, n))
    lx = rng.normal(-np.log(n), 1.5, size=(1, n)) + group + rng.uniform(0.1, 0.5, size=(S, 1)) * rng.normal(0, 1, size=(S, n))
    W = rng.normal(0, 0.1, size=(n, C))
    return lx, W


def test_restatement_gradient_matches_central_differences():
    """tests/tsne_restatement.py in float64 at S = 7, n = 130, C = 2, B = 5 with an unsorted batch, bandwidths set explicitly; the two
    samples outside the batch get their gradient through the normaliser of Q alone.  The bias gradient sum_s dz_s is zero."""
    import tsne_restatement as T
    rng = np.random.default_rng(91)
    S, n, C = 7, 130, 2
    lx, W = _problem(rng, S, n, C)
    batch = np.array([4, 0, 6, 1, 3])
    delta = T.pairwise_delta(lx)
    sig = np.sqrt(np.median(delta[delta > 0])) * rng.uniform(0.3, 0.8, size=S)
    for use_vlr, alpha in ((True, 1.0), (False, 2.5)):
        sg = sig if use_vlr else sig * np.sqrt(n)
        loss, g_W, dz, P, Q = T.loss_and_gradient(W, lx, batch, sg, use_vlr, alpha)
        assert loss == T.loss(W, lx, batch, sg, use_vlr, alpha) and loss > 0
        off = P[~np.eye(len(batch), dtype=bool)]
        assert off.max() > 3 * off.min()  # (P is far from uniform: the distances matter)
        assert np.abs(dz[[2, 5]]).min() > 0  # (samples outside the batch)
        assert np.abs(dz.sum(axis=0)).max() <= 1e-12 * np.abs(dz).sum()
        h, scale = 1e-5, np.abs(g_W).max()
        for idx in np.ndindex(*W.shape):
            keep = W[idx]
            W[idx] = keep + h
            up = T.loss(W, lx, batch, sg, use_vlr, alpha)
            W[idx] = keep - h
            dn = T.loss(W, lx, batch, sg, use_vlr, alpha)
            W[idx] = keep
            fd = (up - dn) / (2 * h)
            assert abs(g_W[idx] - fd) <= 1e-5 * abs(fd) + 1e-6 * scale, (idx, g_W[idx], fd)


def test_restatement_distances_p_and_q():
    import tsne_restatement as T
    rng = np.random.default_rng(92)
    lx, W = _problem(rng, 6, 40, 3)
    d = T.pairwise_delta(lx)
    np.testing.assert_array_equal(d, d.T)
    assert not np.diag(d).any()
    np.testing.assert_allclose(d[1, 4], np.var(lx[1] - lx[4]), rtol=1e-13)
    np.testing.assert_allclose(T.pairwise_delta(lx, False)[1, 4], ((lx[1] - lx[4]) ** 2).sum(), rtol=1e-13)
    # (a shift of one whole row -- another sequencing depth in log space -- leaves the variance of the log-ratio alone)
    lx2 = lx.copy()
    lx2[2] += 3.0
    np.testing.assert_allclose(T.pairwise_delta(lx2), d, rtol=1e-10, atol=1e-13)
    sig = np.full(6, np.sqrt(np.median(d[d > 0])))
    P = T.p_matrix(d, sig, 6, eps=0.0)
    np.testing.assert_allclose(P.sum(), 1.0, rtol=1e-12)  # (B = S: the column-normalised halves sum to S / (2 S) each)
    np.testing.assert_array_equal(P, P.T)
    Q = T.q_matrix(lx @ W)
    np.testing.assert_allclose(Q.sum(), 1.0, rtol=1e-12)
    assert not np.diag(Q).any()
    p, m, v = T.adam_step(np.array([1.0, -2.0]), np.array([0.5, -4.0]), 0.0, 0.0, 1, 1e-2)
    np.testing.assert_allclose(p, [1.0 - 1e-2, -2.0 + 1e-2], rtol=0, atol=1e-8)  # (the first step is lr, whatever the gradient)
    np.testing.assert_allclose(T.embed(W, [lx, lx + 2.0]), (lx + 1.0) @ W, rtol=1e-12)


def test_find_sigmas_honours_the_bracket_and_reaches_the_perplexity():
    """S = 60, n = 50: the target 50 is below S - 1, so the bisection converges: sigma stays in [1e-2, 10 sqrt(max delta)] and the
    target lies between the perplexities one final bracket width (2^-20 of the first) below and above it."""
    import tsne_restatement as T
    from polee_amd import tsne
    rng = np.random.default_rng(93)
    S, n = 60, 50
    lx = _problem(rng, S, n, 1)[0]
    delta = T.pairwise_delta(lx)
    target = min(50.0, S - 1.0)
    sig, lo0, hi0 = T.find_sigmas(delta, target)
    np.testing.assert_array_equal(tsne.find_sigmas(delta, target), sig.astype(np.float32))
    assert (sig > lo0).all() and (sig < hi0).all()
    np.testing.assert_allclose(hi0, 10.0 * np.sqrt(delta.max(axis=1)), rtol=1e-15)
    for i in range(S):
        w = (hi0[i] - lo0[i]) * 2.0 ** -20
        assert T.perplexity(delta[i], i, sig[i] - w) <= target <= T.perplexity(delta[i], i, sig[i] + w), i
        assert abs(T.perplexity(delta[i], i, sig[i]) - target) < 1e-3


def test_find_sigmas_at_the_largest_possible_target_ends_at_the_top_of_the_bracket():
    """S = 5: the target is S - 1, which only a uniform row reaches, so every step raises lo"""
    import tsne_restatement as T
    rng = np.random.default_rng(94)
    S = 5
    delta = T.pairwise_delta(_problem(rng, S, 50, 1)[0])
    sig, lo0, hi0 = T.find_sigmas(delta, min(50.0, S - 1.0))
    assert (sig < hi0).all() and (sig >= hi0 - (hi0 - lo0) * 2.0 ** -20).all()


def test_w0_and_the_minibatches_follow_from_the_seed():
    from polee_amd import tsne
    w = tsne.initial_weights(7, 33, 3)
    assert w.dtype == np.float32 and w.shape == (33, 3)
    np.testing.assert_array_equal(w, np.random.default_rng([7, 0]).normal(0.0, 1e-4, (33, 3)).astype(np.float32))
    np.testing.assert_array_equal(w, tsne.initial_weights(7, 33, 3))
    assert not np.array_equal(w, tsne.initial_weights(8, 33, 3))
    assert 0.5e-4 < w.std() < 2e-4
    b = tsne.minibatches(7, 12, 5, 6)
    assert b.dtype == np.int32 and b.shape == (6, 5)
    rng = np.random.default_rng([7, 1])
    np.testing.assert_array_equal(b, np.array([rng.permutation(12)[:5] for _ in range(6)]))
    np.testing.assert_array_equal(b, np.concatenate([tsne.minibatches(7, 12, 5, 2), tsne.minibatches(7, 12, 5, 4, first=2)]))
    assert all(len(set(row)) == 5 and min(row) >= 0 and max(row) < 12 for row in b.tolist())
    assert not np.array_equal(b, tsne.minibatches(8, 12, 5, 6))
    assert sorted(tsne.minibatches(7, 12, 12, 1)[0].tolist()) == list(range(12))  # (B = S: a permutation)

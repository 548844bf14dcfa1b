"""Host side of `polee model regression` (polee_amd/regression.py; src/regression.jl, src/PoleeModel.jl:165-263,
src/rnaseq_sample.jl:229-250, src/estimate.jl:66-146): the design matrix, the gene bookkeeping, the writers, the kallisto loader, the
command line's option checks, and self-checks of the restatement the GPU tests compare against.  No GPU."""
import json

import numpy as np
import pytest

NEW_SYMBOLS = ["polee_effects_create", "polee_effects_destroy", "polee_effects_run"]
FACTORS = [{"tissue": "liver", "sex": "f"}, {"tissue": "brain", "sex": "m"}, {"tissue": "liver"}, {"tissue": "brain", "sex": "f"}]


def test_the_library_exports_the_symbols_and_the_package_the_names():
    import polee_amd
    from polee_amd import regression as R
    lib = polee_amd.lib()
    assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    for name in ("IsoformEffects", "estimate_isoform_effect_sizes", "build_design_matrix", "gene_map", "gene_initial_values",
                 "write_isoform_regression_effects", "write_aitchison_results", "write_expression", "load_kallisto_estimates"):
        assert getattr(polee_amd, name) is getattr(R, name)
    assert callable(R.main) and callable(R.parser)


# ---- build_design_matrix
def test_design_matrix_of_two_factors_in_sorted_order_with_a_missing_option():
    from polee_amd.regression import build_design_matrix
    F, names = build_design_matrix(FACTORS)
    assert names == ["sex:f", "sex:m", "sex:missing", "tissue:brain", "tissue:liver"]
    assert F.dtype == np.float32
    np.testing.assert_array_equal(F, [[1, 0, 0, 0, 1], [0, 1, 0, 1, 0], [0, 0, 1, 0, 1], [1, 0, 0, 1, 0]])


def test_design_matrix_nonredundant_in_its_three_forms():
    from polee_amd.regression import build_design_matrix
    F, names = build_design_matrix(FACTORS, nonredundant="")  # "missing" where present, else the first sorted option
    assert names == ["sex:f", "sex:m", "tissue:liver"]
    np.testing.assert_array_equal(F, [[1, 0, 1], [0, 1, 0], [0, 0, 1], [1, 0, 0]])
    F, names = build_design_matrix(FACTORS, nonredundant="liver")  # a named option, dropped where it occurs
    assert names == ["sex:f", "sex:m", "sex:missing", "tissue:brain"]
    np.testing.assert_array_equal(F[:, 3], [0, 1, 0, 1])
    assert build_design_matrix(FACTORS, nonredundant=None)[1] == build_design_matrix(FACTORS)[1]


def test_design_matrix_balanced_and_a_subset_of_factors():
    from polee_amd.regression import build_design_matrix
    F, names = build_design_matrix(FACTORS, factors=["tissue"], balanced=True)
    assert names == ["tissue:brain", "tissue:liver"]
    np.testing.assert_array_equal(F, [[-1, 1], [1, -1], [-1, 1], [1, -1]])
    F, names = build_design_matrix(FACTORS, factors=["tissue", "sex"], nonredundant="")
    assert names == ["sex:f", "sex:m", "tissue:liver"]  # (sorted, whatever order --factors names them in)


# ---- gene_map
IDS = ["G1.t1", "G2.t1", "G1.t2", "orphan", "G3.t1", "G2.t2", "other"]


def test_gene_map_by_pattern_with_and_without_a_capture_group():
    from polee_amd.regression import gene_map
    G, gi, ti, gene_ids, gene_names = gene_map(IDS, pattern=r"^(G\d+)\.")
    assert G == 5 and gene_ids == ["G1", "G2", "unknown-gene-1", "G3", "unknown-gene-2"]  # first appearance; unmatched: genes of their own
    np.testing.assert_array_equal(gi, [1, 2, 1, 3, 4, 2, 5])
    np.testing.assert_array_equal(ti, np.arange(1, 8))
    assert gene_names == [""] * 5
    G, gi, _, gene_ids, _ = gene_map(IDS, pattern=r"G\d+")  # no capture group: the whole match
    assert gene_ids == ["G1", "G2", "unknown-gene-1", "G3", "unknown-gene-2"]
    G, gi, _, gene_ids, _ = gene_map(IDS, pattern=r"t\d")  # searched anywhere in the id, as Julia's match
    assert gene_ids == ["t1", "t2", "unknown-gene-1", "unknown-gene-2"]
    np.testing.assert_array_equal(gi, [1, 1, 2, 3, 1, 2, 4])


def test_gene_map_from_an_annotations_file(tmp_path):
    from polee_amd.pca import read_experiment
    from polee_amd.regression import gene_map
    ann = [{"gene_name": "B", "transcripts": ["t2", "t4"]}, {"gene_name": "A", "transcripts": ["t1", "t3", 5]}]
    (tmp_path / "genes.yml").write_text(json.dumps(ann))
    G, gi, ti, gene_ids, _ = gene_map(["t1", "t2", "t3", "t4", "5"], annotations=read_experiment(str(tmp_path / "genes.yml")))
    assert G == 2 and gene_ids == ["A", "B"]
    np.testing.assert_array_equal(gi, [1, 2, 1, 2, 1])
    with pytest.raises(ValueError, match="t9"):
        gene_map(["t1", "t9"], annotations=ann)
    with pytest.raises(ValueError):
        gene_map(["t1"], pattern="t", annotations=ann)


def test_gene_initial_values_against_the_loop():
    from polee_amd.regression import gene_initial_values, gene_map
    rng = np.random.default_rng(3)
    S, n = 3, len(IDS)
    G, gi, ti, _, _ = gene_map(IDS, pattern=r"^(G\d+)\.")
    x = rng.dirichlet(np.ones(n), size=S).astype(np.float32)
    xg, xi = gene_initial_values(gi, ti, x, S, G, n)
    want_g, want_i = np.zeros((S, G), np.float32), np.zeros((S, n), np.float32)
    for i in range(S):  # (src/PoleeModel.jl:246-260, written out)
        for j, k in zip(gi, ti):
            want_g[i, j - 1] += x[i, k - 1]
            want_i[i, k - 1] = x[i, k - 1]
        for j, k in zip(gi, ti):
            want_i[i, k - 1] /= want_g[i, j - 1]
            want_i[i, k - 1] = np.log(want_i[i, k - 1])
        for j in range(G):
            want_g[i, j] = np.log(want_g[i, j])
    assert xg.dtype == np.float32 and xi.dtype == np.float32
    np.testing.assert_allclose(xg, want_g, rtol=3e-7, atol=3e-7)  # (one ulp of logf: NumPy's array and scalar logs may differ by it)
    np.testing.assert_allclose(xi, want_i, rtol=3e-7, atol=3e-7)
    assert (xi[:, 3] == 0).all()  # (a gene of one isoform: log 1)


# ---- writers
def test_isoform_and_aitchison_writers(tmp_path):
    from polee_amd.regression import write_aitchison_results, write_isoform_regression_effects
    gi, ti = np.array([1, 2, 1]), np.array([1, 2, 3])
    mn = np.array([[0.5, 0.0, 1.25e-5]], np.float32)
    me = np.array([[-0.5, 0.0, 3.0e6]], np.float32)
    pr = np.array([[0.25, 0.0, 1.0]], np.float32)
    fn = str(tmp_path / "iso.csv")
    write_isoform_regression_effects(fn, gi, ti, ["tissue:liver"], ["gA", "gB"], ["", "nameB"], ["t1", "t2", "t3"], mn, me, pr,
                                     np.array([[0.1, 0.2, 0.3]], np.float32), np.array([-1.0, -2.0, -3.5], np.float32),
                                     np.array([0.5, 0.25, 0.125], np.float32))
    rows = open(fn).read().splitlines()
    assert rows[0] == "factor,gene_id,gene_name,transcript_id,mean_effect_size,min_effect_size,prob_de,w_mean,x_bias,x_scale"
    assert rows[1] == "tissue:liver,gA,,t1,-0.5,0.5,0.25,0.1,-1.0,0.5"
    assert rows[2] == "tissue:liver,gB,nameB,t2,0.0,0.0,0.0,0.2,-2.0,0.25"
    assert rows[3] == "tissue:liver,gA,,t3,3.0e6,1.25e-5,1.0,0.3,-3.5,0.125"  # (print(::Float32) of Julia)
    write_isoform_regression_effects(fn, gi, ti, ["tissue:liver"], ["gA", "gB"], ["", "nameB"], ["t1", "t2", "t3"], mn, me, None,
                                     np.array([[0.1, 0.2, 0.3]], np.float32), np.array([-1.0, -2.0, -3.5], np.float32),
                                     np.array([0.5, 0.25, 0.125], np.float32))
    rows = open(fn).read().splitlines()
    assert rows[0] == "factor,gene_id,gene_name,transcript_id,mean_effect_size,min_effect_size,w_mean,x_bias,x_scale"
    assert rows[1] == "tissue:liver,gA,,t1,-0.5,0.5,0.1,-1.0,0.5" and len(rows) == 4
    fn = str(tmp_path / "ait.csv")
    write_aitchison_results(fn, ["a:x", "a:y"], ["gA", "gB"], ["", "nameB"], np.array([[0.5, 0.25], [1, 2]], np.float32),
                            np.array([[1.5, 0.75], [3, 4]], np.float32), np.array([[0.125, 1.0], [0, 0.5]], np.float32))
    rows = open(fn).read().splitlines()
    assert rows[0] == "factor,gene_id,gene_name,mean_effect_size,min_effect_size,prob_de" and len(rows) == 5
    assert rows[1] == "a:x,gA,,1.5,0.5,0.125" and rows[4] == "a:y,gB,nameB,4.0,2.0,0.5"
    write_aitchison_results(fn, ["a:x"], ["gA"], [""], np.array([[0.5]], np.float32), np.array([[1.5]], np.float32), None)
    assert open(fn).read().splitlines() == ["factor,gene_id,gene_name,mean_effect_size,min_effect_size", "a:x,gA,,1.5,0.5"]


def test_expression_and_initial_value_writers(tmp_path):
    from polee_amd.regression import write_expression, write_x_init
    fn = str(tmp_path / "expr.csv")
    qx = np.log(np.array([[0.25, 0.75], [0.5, 0.5]], np.float32))
    write_expression(fn, "transcript_id", ["t1", "t2"], ["s1", "s2"], qx)
    rows = open(fn).read().splitlines()
    assert rows[0] == "transcript_id,sample,tpm"
    assert [r.rsplit(",", 1)[0] for r in rows[1:]] == ["t1,s1", "t1,s2", "t2,s1", "t2,s2"]  # (feature-major, :579)
    np.testing.assert_allclose([float(r.rsplit(",", 1)[1]) for r in rows[1:]], [250000.0, 500000.0, 750000.0, 500000.0], rtol=1e-6)
    write_x_init(fn, "gene_id", ["gA", "gB"], qx)
    rows = open(fn).read().splitlines()
    assert rows[0] == "gene_id,x1,x2" and [r.split(",")[0] for r in rows[1:]] == ["gA", "gB"]
    np.testing.assert_allclose([[float(v) for v in r.split(",")[1:]] for r in rows[1:]], [[0.25, 0.5], [0.75, 0.5]], rtol=1e-6)


# ---- kallisto
def _kallisto_file(path, ids, efflens, counts, bootstraps=()):
    from polee_amd import h5io
    with h5io.File(path, "w") as f:
        f.create_group("aux")
        f.write("aux/eff_lengths", np.asarray(efflens, np.float64))
        f.write_strings("aux/ids", ids)
        f.write("est_counts", np.asarray(counts, np.float64))
        if len(bootstraps):
            f.create_group("bootstrap")
            for b, bs in enumerate(bootstraps):
                f.write("bootstrap/bs%d" % b, np.asarray(bs, np.float64))


def test_kallisto_loader_with_and_without_bootstrap(tmp_path):
    from polee_amd.regression import load_kallisto_estimates
    ids = ["t1", "t2", "t3"]
    eff = np.array([100.0, 200.0, 400.0])
    counts = np.array([10.0, 40.0, 40.0])
    bs = np.array([[10.0, 40.0, 40.0], [40.0, 30.0, 40.0], [2.0, 45.0, 40.0], [10.0, 41.0, 39.0]])
    fn = str(tmp_path / "abundance.h5")
    _kallisto_file(fn, ids, eff, counts, bs)
    x0, std = load_kallisto_estimates([fn, fn], pseudocount=1.0)
    assert std is None and x0.shape == (2, 3) and x0.dtype == np.float32
    want = (counts / eff) / (counts / eff).sum() + 1e-6
    np.testing.assert_allclose(x0[0], want, rtol=1e-6)
    x0, std = load_kallisto_estimates([fn], pseudocount=1.0, use_bootstrap=True)
    props = bs / eff
    logp = np.log(props / props.sum(axis=1, keepdims=True) + 1e-6)
    np.testing.assert_allclose(x0[0], np.exp(logp.mean(axis=0)), rtol=1e-5)
    np.testing.assert_allclose(std[0], np.maximum(0.5, logp.std(axis=0, ddof=1)), rtol=1e-4)
    assert std[0, 2] == 0.5 and std[0, 0] > 0.5  # (the floor holds for the steady transcript, not for the noisy one)
    # rows placed by transcript id: another order, and a transcript the file does not know
    x0, _ = load_kallisto_estimates([fn], transcript_ids=["t3", "tX", "t1", "t2"])
    np.testing.assert_allclose(x0[0], [want[2] - 1e-6, 0.0, want[0] - 1e-6, want[1] - 1e-6], rtol=1e-5, atol=1e-9)
    _kallisto_file(fn, ids, eff, counts, bs[:1])
    with pytest.raises(ValueError, match="bootstrap"):
        load_kallisto_estimates([fn], use_bootstrap=True)


# ---- the command line: every option conflict exits with its message before anything touches a device
CONFLICTS = [
    (["--feature", "exon"], "exon is not a supported feature."),
    (["--feature", "splice-feature"], "splice-feature is not built"),
    (["--gene-pattern", "x", "--gene-annotations", "g.yml"], "At most one of --gene-pattern and --gene-annotations can be given."),
    (["--kallisto", "--kallisto-bootstrap"], "Only one of '--kallisto' and '--kallisto-bootstrap' can be used."),
    (["--kallisto", "--point-estimates", "tpm"], "'--use-point-estimates' in not compatible with '--kallisto' or '--kallisto-bootstrap'"),
    (["--kallisto-bootstrap", "--point-estimates", "tpm"], "'--use-point-estimates' in not compatible with '--kallisto' or '--kallisto-bootstrap'"),
    (["--pseudocount", "1"], "--pseudocount argument only valid with --point-estimates"),
    (["--feature", "gene", "--gene-pattern", "x", "--kallisto-bootstrap"], "gene regression with --kallisto-bootstrap not yet implemented"),
    (["--feature", "gene-isoform", "--gene-pattern", "x", "--kallisto-bootstrap"],
     "gene-isoform regression with --kallisto-bootstrap not yet implemented"),
    (["--feature", "gene", "--gene-pattern", "x", "--kallisto"], "gene regression is built on the approximate likelihood only"),
    (["--feature", "gene-isoform", "--gene-pattern", "x", "--point-estimates", "tpm"],
     "gene-isoform regression is built on the approximate likelihood only"),
    (["--feature", "gene"], "--feature gene needs --gene-pattern or --gene-annotations"),
    (["--point-estimates", "tpm"], "--point-estimates needs --transcript-ids"),
    (["--num-steps", "0"], "--num-steps and --effect-draws must be positive"),
    (["--feature", "gene-isoform", "--gene-pattern", "x", "--effect-draws", "0"], "--num-steps and --effect-draws must be positive"),
]


@pytest.mark.parametrize("argv,message", CONFLICTS)
def test_option_conflicts_exit_with_their_message(argv, message):
    from polee_amd import regression
    with pytest.raises(SystemExit) as ei:
        regression.main(["no-such-experiment.yml"] + argv)
    assert message in str(ei.value.code)


def test_parser_defaults_are_the_references():
    from polee_amd import regression
    a = regression.parser().parse_args(["e.yml"])
    assert (a.feature, a.output, a.isoform_output) == ("transcript", "regression-coefficients.csv", "regression-isoform-coefficients.csv")
    assert (a.lower_credible, a.upper_credible, a.min_effect_size_coverage, a.scale_penalty) == (0.025, 0.975, 0.1, 1e-3)
    assert a.aitchison_distance_effect_size == 1.0 and a.effect_size is None and a.isoform_effect_size is None
    assert a.redundant_factor == "" and not a.nonredundant and not a.balanced and a.effect_draws == 1000 and a.num_steps is None
    assert regression.NUM_STEPS == {"transcript": 6000, "gene": 10000, "gene-isoform": 6000}


# ---- the restatement
def test_restatement_aitchison_distance_is_the_within_gene_std_of_w():
    import isoform_effects_restatement as T
    rng = np.random.default_rng(9)
    n, G, F, niter = 40, 7, 2, 6
    gene_of = rng.permutation(np.concatenate([np.arange(G), rng.integers(0, G, size=n - G)]))
    qw_loc, qw_scale = rng.normal(0, 1, (F, n)), np.exp(rng.normal(-1.5, 0.7, (F, n)))
    loc, scale = rng.normal(-2, 3, n), np.exp(rng.normal(-1.5, 0.7, n))
    zx, zw = rng.normal(size=(niter, n)), rng.normal(size=(niter, F, n))
    e, a = T.effect_size_samples(gene_of, G, qw_loc, qw_scale, loc, scale, zx, zw)
    w = zw * qw_scale + qw_loc  # [niter, F, n]
    x = zx * scale + loc
    for g in range(G):
        idx = np.nonzero(gene_of == g)[0]
        np.testing.assert_allclose(a[:, g, :], w[:, :, idx].std(axis=2).T, rtol=2e-6, atol=1e-7)  # (a is stored as Float32)
        for i in range(F):  # and e is w - (lse(x + w) - lse(x)) over the gene
            v = x[:, idx] + w[:, i, idx]
            d = np.log(np.exp(v).sum(axis=1)) - np.log(np.exp(x[:, idx]).sum(axis=1))
            np.testing.assert_allclose(e[i, idx, :].T, w[:, i, idx] - d[:, None], rtol=2e-6, atol=2e-6)


def test_restatement_single_isoform_genes_and_the_order_statistic():
    import isoform_effects_restatement as T
    rng = np.random.default_rng(10)
    n, F, niter = 6, 2, 25
    zx, zw = rng.normal(size=(niter, n)), rng.normal(size=(niter, F, n))
    out = T.estimate_isoform_effect_sizes(np.arange(n), n, 0.4, 0.5, rng.normal(0, 1, (F, n)), np.ones((F, n)), rng.normal(-2, 3, n),
                                          np.ones(n), zx, zw)
    for r in out:
        assert not r.any()  # e = log 1 - log 1 = 0 and a = 0, exactly
    assert T.order_statistic_index(25, 0.1) == 2    # round(2.5) = 2: half to even
    assert T.order_statistic_index(5, 0.1) == 1     # round(0.5) = 0, clamped
    assert T.order_statistic_index(1000, 0.1) == 100 and T.order_statistic_index(1, 0.1) == 1 and T.order_statistic_index(7, 1.0) == 7
    xs = np.array([-3.0, 0.5, 2.0, -0.25, 1.0])
    assert T.find_minimum_effect_size_from_samples(xs, 0.1) == 0.25 and T.find_minimum_effect_size_from_samples(xs, 0.5) == 0.5
    assert T.estimate_isoform_effect_sizes(np.arange(n), n, None, None, np.zeros((F, n)), np.ones((F, n)), np.zeros(n), np.ones(n), zx, zw)[2] is None

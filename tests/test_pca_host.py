"""Host side of `polee model pca` (polee_amd/pca.py; models/pca.jl, models/polee_pca.py): command line, the two CSV writers, and
the restatement the GPU tests compare against (its analytic z-gradient against central differences).  No GPU."""
import json

import numpy as np
import pytest

from oracle import regression_ref as RR


def test_rnaseq_pca_is_exported():
    import polee_amd
    from polee_amd.pca import RNASeqPCA
    assert polee_amd.RNASeqPCA is RNASeqPCA
    assert issubclass(RNASeqPCA, polee_amd.RNASeqLinearRegression)
    for name in ("set_latent_design", "get_design"):
        assert callable(getattr(polee_amd.RNASeqLinearRegression, name))


def test_the_library_exports_the_two_symbols():
    import polee_amd
    lib = polee_amd.lib()
    assert lib.polee_regression_set_latent_design and lib.polee_regression_get_design


def test_cli_parsing_defaults_and_options():
    from polee_amd import pca
    a = pca.parser().parse_args(["experiment.yml"])
    assert (a.experiment, a.feature, a.num_components, a.output_z, a.output_w) == ("experiment.yml", "transcript", 2, "pca-z.csv", None)
    assert (a.num_steps, a.seed, a.device, a.max_num_samples, a.transcript_ids, a.point_estimates) == (12000, 123456789, 0, None, None,
                                                                                                       None)
    a = pca.parser().parse_args(["e.yml", "--num-components", "5", "--output-z", "z.csv", "--output-w", "w.csv", "--num-steps", "10",
                                 "--seed", "3", "--device", "1", "--max-num-samples", "4", "--transcript-ids", "ids.txt"])
    assert (a.num_components, a.output_z, a.output_w, a.num_steps, a.seed, a.device, a.max_num_samples, a.transcript_ids) == \
        (5, "z.csv", "w.csv", 10, 3, 1, 4, "ids.txt")
    with pytest.raises(SystemExit):
        pca.parser().parse_args([])


@pytest.mark.parametrize("argv,needle", [(["e.yml", "--feature", "isoform"], "--feature isoform is not built"),
                                         (["e.yml", "--point-estimates", "kallisto"], "--point-estimates is not built"),
                                         (["e.yml", "--feature", "gene"], "gene is not a supported feature"),
                                         (["e.yml", "--num-components", "17"], "--num-components must be 1..16")])
def test_cli_refuses_what_is_not_built(argv, needle):
    from polee_amd import pca
    with pytest.raises(SystemExit) as ei:  # (before the experiment file is opened: e.yml does not exist)
        pca.main(argv)
    assert needle in str(ei.value.code)


def test_experiment_file_is_yaml_or_json(tmp_path):
    from polee_amd import pca
    spec = {"samples": [{"name": "a", "file": "a.h5"}, {"name": "b", "file": "b.h5"}]}
    f = tmp_path / "experiment.yml"
    f.write_text(json.dumps(spec))  # (JSON is YAML: both parsers read it)
    assert pca.read_experiment(str(f)) == spec
    try:
        import yaml  # noqa: F401
    except ImportError:
        f.write_text("samples:\n  - name: a\n")
        with pytest.raises(SystemExit) as ei:
            pca.read_experiment(str(f))
        assert "yaml module is not installed" in str(ei.value.code)


def test_csv_writers_byte_for_byte(tmp_path):
    """write_pca_z / write_pca_w (models/pca.jl:179-223): header, one row per sample / per transcript, values as Julia prints Float32
    (shortest round-trip digits; exponent form below 1e-4 and from 1e6)."""
    from polee_amd import pca
    z = np.array([[0.5, -1.25, 1e-5], [3.0, 0.1, 1234567.0]], np.float32)
    pca.write_pca_z(str(tmp_path / "z.csv"), ["s1", "s2"], z)
    assert (tmp_path / "z.csv").read_bytes() == (b"sample,component1,component2,component3\n"
                                                 b"s1,0.5,-1.25,1.0e-5\n"
                                                 b"s2,3.0,0.1,1.234567e6\n")
    w = np.array([[0.5, -1.25, 0.0001], [3.0, 0.1, -2.5e-7]], np.float32)  # [C = 2][n = 3]
    pca.write_pca_w(str(tmp_path / "w.csv"), ["t1", "t2", "t3"], w)
    assert (tmp_path / "w.csv").read_bytes() == (b"transcript_id,component1,component2\n"
                                                 b"t1,0.5,3.0\n"
                                                 b"t2,-1.25,0.1\n"
                                                 b"t3,0.0001,-2.5e-7\n")
    with pytest.raises(ValueError):
        pca.write_pca_z(str(tmp_path / "bad.csv"), ["s1"], z)
    with pytest.raises(ValueError):
        pca.write_pca_w(str(tmp_path / "bad.csv"), ["t1"], w)


def test_restatement_z_gradient_matches_central_differences():
    """pca_loss of tests/pca_restatement.py (what tests/test_gpu_pca.py holds the device to) in float64 at S = 3, n = 40: point
    estimates and a surrogate draw of x, no likelihood term (it does not depend on z)."""
    import pca_restatement as T
    rng = np.random.default_rng(61)
    S, Cdim, n, deg, sigma = 3, 2, 40, 4, 1.7
    x_init = (rng.normal(-np.log(n), 1.5, size=(1, n)) + rng.normal(0, 0.4, size=(S, n))).astype(np.float32)
    W = T.weights(x_init, deg, 1.0)
    ss = rng.normal(0, 0.2, size=(S, 1))
    p0 = RR.flatten(RR.initial_params(x_init, Cdim, deg), RR.PARAMS)
    p = RR.unflatten(p0 + rng.normal(0, 0.3, size=p0.size), RR.PARAMS, S, Cdim, n, deg)
    e = RR.unflatten(rng.normal(size=2 + 5 * Cdim * n + 2 * n + S * n), RR.NOISE, S, Cdim, n, deg)
    z = rng.normal(0, 0.7, size=(S, Cdim))
    for point, dist in ((True, True), (False, False)):
        common = dict(W=W, sample_scales=ss, x_bias_loc0=np.log(1.0 / n), x_bias_scale0=12.0, use_distortion=dist, scale_penalty=0.7,
                      use_point_estimates=point)
        loss, draws = T.pca_loss(p, e, z, sigma, **common)
        assert abs(loss - RR.regression_loss(p, e, design=z, **common)[0] - T.prior_nlp(z, sigma)) < 1e-9 * abs(loss)
        g = T.pca_z_gradient(p, draws, z, sigma, W, ss, dist)
        h = 1e-4
        for s in range(S):
            for f in range(Cdim):
                zp, zm = z.copy(), z.copy()
                zp[s, f] += h
                zm[s, f] -= h
                fd = (T.pca_loss(p, e, zp, sigma, **common)[0] - T.pca_loss(p, e, zm, sigma, **common)[0]) / (2 * h)
                assert abs(g[s, f] - fd) <= 1e-6 * (abs(fd) + np.abs(g).max()), (s, f, g[s, f], fd)

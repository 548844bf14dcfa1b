"""polee_amd -- host side of the MI355X approximate-likelihood engine for Polee.

A Python mirror of the reference's Julia interface for the hot path (Julia is not
available in the build image; julia/PoleeHIP.jl holds the ccall wrappers a maintainer
would use).  Names, argument meaning and error behaviour follow the reference:

  PolyaTreeTransform, transform!, transform_gradients!, inverse_transform!   src/ptt.jl
  make_inverse_ptt_params                                                    src/ptt.jl:293-309
  hsb / inv_hsb / inv_hsb_grad  (TF custom ops)                              src/tensorflow_ext/hsb_ops.cpp
  RNASeqSample.X + log_likelihood / factored_log_likelihood                  src/likelihood.jl
  approximate_likelihood(LogitSkewNormalPTTApprox(), sample)                 src/likelihood-approximation.jl
  approximate_likelihood(LogisticNormalApprox() | NormalILRApprox() | NormalALRApprox(), sample)
  (`prep --approx-method`)                                                   src/likelihood-approximation-alt.jl
  sample_likap                                                               src/evaluate.jl:8-275
  ApproxLikelihoodSampler / rand!                                            src/approx-sampler.jl
  RNASeqApproxLikelihood(...).log_prob, rnaseq_approx_likelihood_sampler     src/polee_approx_likelihood.py
  RNASeqLinearRegression / RNASeqTranscriptLinearRegression(...).fit         models/polee_regression.py
  estimate_isoform_effect_sizes, build_design_matrix, gene_map               src/regression.jl, src/PoleeModel.jl:165-263
  (`polee model regression`: python -m polee_amd.regression)
  RNASeqPCA(...).fit (`polee model pca`)                                     models/polee_pca.py, models/pca.jl
  RNASeqLogisticRegression (`polee model classify`)                          models/polee_classify.py, models/classify.jl
  RNASeqTSNE, estimate_tsne (`polee model tsne`)                             models/polee_tsne.py, models/tsne.jl
  RNASeqRandomForest (`polee model random-forest`)                           models/random-forest.jl
  build_likelihood_matrix (X from alignments, SimplisticFragModel)           src/rnaseq_sample.jl:58-121, src/fragmodel.jl
  gibbs_sampler / GibbsSampler (`polee debug-sample`)                        src/gibbs.jl, src/main.jl:925-957
  expectation_maximization / EM (`polee debug-optimize`)                     src/em.jl, src/main.jl:960-988
  polee_sample / ApproxSampleStream / multinomial_counts (`polee sample`)    src/main.jl:756-919
  read_fasta / kmer_sketches / build_polya_tree_transformation               src/kmersketch.jl, src/kmercluster.jl
  (`polee fit-tree`: python -m polee_amd.fit_tree)                           src/main.jl:638-660
  train_bias_model / fragment_length_model (BiasModel, BiasedFragModel)      src/bias.jl:266-828, src/fragmodel.jl:263-343
  (python -m polee_amd.bias)
  train_fragment_model / estimate_simplistic / assign_reads                   src/rnaseq_sample.jl:330-380, src/fragmodel.jl:35-113, :186-293
  (python -m polee_amd.fragmodel)

All numerics run in libpolee_hip.so on the GPU; nothing here computes on the CPU.
"""
from ._lib import PoleeError, NonFiniteError, lib, LIB_PATH  # noqa: F401
from .core import (Context, Comm, HostComm, version, hclust, host_cache_trim, sample_and_tree, PolyaTreeTransform, make_inverse_ptt_params, hsb, inv_hsb, inv_hsb_grad,  # noqa: F401
                   RNASeqSample, DeviceX, log_likelihood, factored_log_likelihood,
                   effective_length_jacobian_adjustment, gene_noninformative_prior, LogitSkewNormalPTTApprox, approximate_likelihood,
                   LikelihoodApproximationFit, ApproxLikelihoodSampler, RNASeqApproxLikelihood,
                   rnaseq_approx_likelihood_sampler, LIKAP_NUM_STEPS, LIKAP_NUM_MC_SAMPLES,
                   logit_normal_transform, logit_normal_transform_gradients, sinh_asinh_transform,
                   sinh_asinh_transform_gradients, kumaraswamy_transform, kumaraswamy_transform_gradients,
                   OptimizePTTApprox, optimize_likelihood, list_nodes,
                   LogisticNormalApprox, KumaraswamyPTTApprox, LogitNormalPTTApprox, NormalILRApprox, NormalALRApprox,
                   AltLikelihoodApproximationFit, sample_likap, approximation_type)

from . import h5io, estimate  # noqa: F401,E402
from .estimate import LoadedSamples, load_samples_from_specification, load_samples_hdf5, read_specification  # noqa: F401,E402
from .regression import (RNASeqLinearRegression, RNASeqTranscriptLinearRegression, RNASeqNormalTranscriptLinearRegression, RNASeqGeneLinearRegression, RNASeqGeneIsoformLinearRegression, RNASeqJointLinearRegression, estimate_sample_scales,  # noqa: F401,E402
                         find_minimum_effect_size, write_regression_effects)
from .pca import RNASeqPCA  # noqa: F401,E402
from .salmon import load_salmon_likelihood, SalmonLikelihood  # noqa: F401,E402
from .cohort import approximate_likelihood_cohort, approximate_likelihood_cohort_processes  # noqa: F401,E402
from .xbuild import build_likelihood_matrix  # noqa: F401,E402


def __getattr__(name):
    # (imported on first use: `python -m polee_amd.gibbs` must not find the module already imported by the package)
    if name in ("GibbsSampler", "gibbs_sampler"):
        from . import gibbs
        return getattr(gibbs, name)
    if name in ("EM", "expectation_maximization"):
        from . import em
        return getattr(em, name)
    if name in ("ApproxSampleStream", "polee_sample", "multinomial_counts"):
        from . import sample
        return getattr(sample, name)
    if name in ("RNASeqLogisticRegression", "build_factor_matrix", "write_classification_probs"):
        from . import classify
        return getattr(classify, name)
    if name in ("RNASeqTSNE", "estimate_tsne"):
        from . import tsne
        return getattr(tsne, name)
    if name in ("RNASeqRandomForest", "build_forest_host", "forest_votes_host"):
        from . import random_forest
        return getattr(random_forest, name)
    if name in ("read_fasta", "kmer_sketches", "kmer_tree", "kmer_candidate_edges", "kmer_round_select", "build_polya_tree_transformation"):
        from . import fit_tree
        return getattr(fit_tree, name)
    if name in ("train_bias_model", "train_bias_model_from_examples", "fragment_length_model", "read_reference_dump",
                "bias_training_examples", "bias_candidate_losses"):
        from . import bias
        return getattr(bias, name)
    if name in ("train_fragment_model", "estimate_simplistic", "assign_reads", "subsample_fragments", "fragment_length_model_from_hist"):
        from . import bias, fragmodel
        return getattr(bias if name == "fragment_length_model_from_hist" else fragmodel, name)
    if name in ("IsoformEffects", "estimate_isoform_effect_sizes", "build_design_matrix", "gene_map", "gene_initial_values",
                "write_isoform_regression_effects", "write_aitchison_results", "write_expression", "load_kallisto_estimates"):
        from . import regression
        return getattr(regression, name)
    raise AttributeError("module 'polee_amd' has no attribute %r" % name)

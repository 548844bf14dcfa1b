"""A plain NumPy f64 restatement of estimate_isoform_effect_sizes (src/regression.jl:761-945) in the reference's own form: exp,
normalise, log, clr, sort(abs), half-even round.  The noise comes in as arguments (zx [niter, n], zw [niter, F, n]).  A helper of
tests/test_regression_cli_host.py and tests/test_gpu_isoform_effects.py, not a test file."""
import numpy as np


def order_statistic_index(niter, target_coverage):
    """clamp(round(Int, target_coverage * niter), 1, niter) (:914); Julia's round is half-to-even, as Python's"""
    return int(min(max(round(target_coverage * niter), 1), niter))


def find_minimum_effect_size_from_samples(xs, target_coverage):
    """:912-915"""
    xs = np.sort(np.abs(xs))
    return xs[order_statistic_index(len(xs), target_coverage) - 1]


def aitchison_distance(xs, ys):
    """:918-945"""
    lx, ly = np.log(xs), np.log(ys)
    return np.sqrt((((lx - lx.mean()) - (ly - ly.mean())) ** 2).sum() / len(xs))


def effect_size_samples(gene_of, num_genes, qw_loc, qw_scale, qx_bias_loc, qx_bias_scale, zx, zw):
    """The per-draw values (:805-866): e Float32 [F, n, niter], a Float32 [F, G, niter] (the reference stores them as Float32)"""
    gene_of = np.asarray(gene_of).reshape(-1)
    qw_loc, qw_scale = np.asarray(qw_loc, np.float64), np.asarray(qw_scale, np.float64)
    loc, scale = np.asarray(qx_bias_loc, np.float64), np.asarray(qx_bias_scale, np.float64)
    F, n = qw_loc.shape
    niter = zx.shape[0]
    genes = [np.nonzero(gene_of == g)[0] for g in range(num_genes)]
    e = np.zeros((F, n, niter), np.float32)
    a = np.zeros((F, num_genes, niter), np.float32)
    for t in range(niter):
        x = np.asarray(zx[t], np.float64) * scale + loc
        p = np.zeros(n)
        for idx in genes:
            if idx.size:
                ex = np.exp(x[idx])
                p[idx] = ex / ex.sum()
        for i in range(F):
            w = np.asarray(zw[t, i], np.float64) * qw_scale[i] + qw_loc[i]
            p_alt = np.zeros(n)
            for idx in genes:
                if idx.size:
                    ex = np.exp(x[idx] + w[idx])
                    p_alt[idx] = ex / ex.sum()
            e[i, :, t] = np.log(p_alt) - np.log(p)
            for g, idx in enumerate(genes):
                if idx.size:
                    a[i, g, t] = aitchison_distance(p[idx], p_alt[idx])
    return e, a


def estimate_isoform_effect_sizes(gene_of, num_genes, effect_size, aitchison_effect_size, qw_loc, qw_scale, qx_bias_loc, qx_bias_scale,
                                  zx, zw, target_coverage=0.1, return_samples=False):
    """(min_effect_sizes, mean_effect_sizes, prob_de, aitchison_min, aitchison_mean, aitchison_prob_de); a prob_de is None when its
    threshold is.  gene_of: the 0-based gene of every transcript.  prob_de is one-sided (e > effect_size, :850), the Aitchison one
    takes |a| (:899)."""
    e, a = effect_size_samples(gene_of, num_genes, qw_loc, qw_scale, qx_bias_loc, qx_bias_scale, zx, zw)
    niter = e.shape[2]
    k = order_statistic_index(niter, target_coverage)
    min_e = np.sort(np.abs(e), axis=2)[:, :, k - 1]
    a_min = np.sort(np.abs(a), axis=2)[:, :, k - 1]
    mean_e, a_mean = e.astype(np.float64).mean(axis=2), a.astype(np.float64).mean(axis=2)
    prob = None if effect_size is None else (e > effect_size).sum(axis=2) / niter
    a_prob = None if aitchison_effect_size is None else (np.abs(a) > aitchison_effect_size).sum(axis=2) / niter
    out = (min_e, mean_e, prob, a_min, a_mean, a_prob)
    return out + (e, a) if return_samples else out

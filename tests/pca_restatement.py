"""The NumPy float64 restatement of the PCA model's loss that tests/test_gpu_pca.py compares the device against, and its analytic
z-gradient (checked against central differences in tests/test_pca_host.py):

    pca_loss(z) = oracle.regression_ref.regression_loss(..., design=z) + sum( z^2 / (2 sigma^2) + log sigma + log(2 pi) / 2 )
"""
import numpy as np

from oracle import regression_ref as RR

HALF_LOG2PI = 0.5 * np.log(2.0 * np.pi)


def weights(x_init, deg, bandwidth):
    mean = x_init.astype(np.float64).mean(axis=0).astype(np.float32).astype(np.float64)
    return RR.kernel_regression_weights(bandwidth, mean, RR.choose_knots(mean.min(), mean.max(), deg))


def prior_nlp(z, sigma):
    return float(np.sum(z * z / (2.0 * sigma * sigma) + np.log(sigma) + HALF_LOG2PI))


def pca_loss(p, e, z, sigma, lik=None, **common):
    """the restatement: (loss, draws)"""
    loss, draws = RR.regression_loss(p, e, design=z, lik=lik, **common)
    return loss + prior_nlp(z, sigma), draws


def pca_z_gradient(p, draws, z, sigma, W, sample_scales, use_distortion):
    w_eff = draws["w"] + (p["qw_distortion_c_loc"] @ W if use_distortion else 0.0)
    mu = draws["x_loc"] - np.asarray(sample_scales, np.float64).reshape(-1, 1)
    a = (draws["x"] - mu) / draws["x_scale"] ** 2
    return -a @ w_eff.T + z / sigma ** 2

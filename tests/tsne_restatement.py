"""Plain NumPy float64 restatement of the parametric t-SNE of `polee model tsne` (models/polee_tsne.py:17-185, :213-398 with
use_vlr=True, alpha=1, no neural network), what tests/test_gpu_tsne.py holds the device to.  A helper module, not a test file.

    z        = lx W                                                      lx [S][n]: log expression (the log of a draw, or points)
    delta_ab = population variance over transcripts of lx_a - lx_b       (use_vlr; else the sum of squares)
    P on the batch I:  E_ab = clip(exp(-delta_ab / (2 sigma_b^2)), 1e-12, 1), E_aa = 0, pc = E / column sums,
                       P = (pc + pc^T) / (2 S) + eps
    Q on all samples:  k_ij = (1 + |z_i - z_j|^2 / alpha)^(-(alpha + 1) / 2), k_ii = 0, Q = k / sum k, gathered to I x I, + eps
    loss     = sum_{a,b in I} P_ab log(P_ab / Q_ab)
"""
import numpy as np


def pairwise_delta(lx, use_vlr=True):
    """delta [B][B] of the rows lx [B][n]"""
    lx = np.asarray(lx, np.float64)
    out = np.zeros((lx.shape[0], lx.shape[0]))
    for a in range(lx.shape[0]):
        d = lx[a][None, :] - lx
        out[a] = d.var(axis=1) if use_vlr else (d * d).sum(axis=1)
    return out


def perplexity(delta_row, i, sigma):
    """2^H of row i at this bandwidth, or None when every e underflows"""
    e = np.exp(-np.asarray(delta_row, np.float64) / (2.0 * sigma * sigma))
    e[i] = 0.0
    tot = e.sum()
    if tot == 0.0:
        return None
    p = e / tot
    p = p[p > 1e-16]
    return 2.0 ** (-(p * np.log2(p)).sum())


def find_sigmas(delta, target, steps=20):
    """per row: lo = 1e-2, hi = 10 sqrt(max_j delta_ij), `steps` bisection steps (a step whose e all underflow raises lo and counts),
    the result (lo + hi) / 2; returns (sigmas, lo0, hi0) with the starting brackets"""
    delta = np.asarray(delta, np.float64)
    S = delta.shape[0]
    sig, lo0, hi0 = np.zeros(S), np.full(S, 1e-2), np.zeros(S)
    for i in range(S):
        lo, hi = 1e-2, 10.0 * np.sqrt(delta[i].max())
        hi0[i] = hi
        for _ in range(steps):
            s = 0.5 * (lo + hi)
            pp = perplexity(delta[i], i, s)
            if pp is None:
                lo = s
            elif pp > target:
                hi = s
            else:
                lo = s
        sig[i] = 0.5 * (lo + hi)
    return sig, lo0, hi0


def p_matrix(delta, sigmas, S, eps=1e-6):
    """delta [B][B] and sigmas [B] of the batch rows; S: ALL samples"""
    sig = np.asarray(sigmas, np.float64)
    E = np.clip(np.exp(-np.asarray(delta, np.float64) / (2.0 * sig[None, :] ** 2)), 1e-12, 1.0)
    np.fill_diagonal(E, 0.0)
    pc = E / E.sum(axis=0)[None, :]
    return (pc + pc.T) / (2.0 * S) + eps


def _kernel(z, alpha):
    d = z[:, None, :] - z[None, :, :]
    D = (d * d).sum(axis=2)
    k = (1.0 + D / alpha) ** (-0.5 * (alpha + 1.0))
    np.fill_diagonal(k, 0.0)
    return d, D, k


def q_matrix(z, alpha=1.0):
    """Q [S][S] without epsilon"""
    k = _kernel(np.asarray(z, np.float64), alpha)[2]
    return k / k.sum()


def loss(W, lx, batch, sigmas, use_vlr=True, alpha=1.0, eps=1e-6):
    lx, W, batch = np.asarray(lx, np.float64), np.asarray(W, np.float64), np.asarray(batch)
    P = p_matrix(pairwise_delta(lx[batch], use_vlr), np.asarray(sigmas, np.float64)[batch], lx.shape[0], eps)
    Q = q_matrix(lx @ W, alpha)[np.ix_(batch, batch)] + eps
    return float((P * np.log(P / Q)).sum())


def loss_and_gradient(W, lx, batch, sigmas, use_vlr=True, alpha=1.0, eps=1e-6):
    """(loss, g_W [n][C], dz [S][C], P [B][B], Q [B][B] with epsilon)"""
    lx, W, batch = np.asarray(lx, np.float64), np.asarray(W, np.float64), np.asarray(batch)
    S = lx.shape[0]
    P = p_matrix(pairwise_delta(lx[batch], use_vlr), np.asarray(sigmas, np.float64)[batch], S, eps)
    z = lx @ W
    d, D, k = _kernel(z, alpha)
    Z = k.sum()
    q = k / Z
    Qb = q[np.ix_(batch, batch)] + eps
    R = np.zeros((S, S))
    R[np.ix_(batch, batch)] = P / Qb
    dLdk = -R / Z + (R * q).sum() / Z
    dkdD = -((alpha + 1.0) / (2.0 * alpha)) * (1.0 + D / alpha) ** (-0.5 * (alpha + 3.0))
    np.fill_diagonal(dkdD, 0.0)  # (k_ii is the constant 0)
    G = dLdk * dkdD
    A = G + G.T
    dz = 2.0 * (A[:, :, None] * d).sum(axis=1)
    return float((P * np.log(P / Qb)).sum()), lx.T @ dz, dz, P, Qb


def adam_step(p, g, m, v, t, lr, b1=0.99, b2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer, step t = 1, 2, ...: returns (p, m, v)"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def embed(W, lx_draws):
    """the mean over the draws of lx W, [S][C]"""
    W = np.asarray(W, np.float64)
    return sum(np.asarray(lx, np.float64) @ W for lx in lx_draws) / len(lx_draws)
